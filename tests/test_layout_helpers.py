"""tests/layout_helpers.py on the CPU: every layout holds the tensor's values in dense planes at the pointer and stride residues
it promises, surrounded by NaN; canary_intact sees a write outside the view, an element left unwritten, a non-finite result."""
import pytest
import torch

from layout_helpers import LAYOUTS, canary_intact, place, place_view

CPU = torch.device("cpu")
SHAPES = [(2, 3, 4, 8), (1, 5, 3, 5), (3, 2, 16), (2, 4, 1, 4), (3, 1, 6, 4)]


def _t(shape):
    return torch.arange(1, 1 + torch.Size(shape).numel(), dtype=torch.float32).view(shape)


def _planes_dense(v):
    exp = 1
    for d in range(v.dim() - 1, 1, -1):
        if v.shape[d] != 1 and v.stride(d) != exp:
            return False
        exp *= v.shape[d]
    return True


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layout_holds_the_values_in_dense_planes_surrounded_by_nan(layout, shape):
    t = _t(shape)
    v, big = place(t, CPU, layout)
    n, c = shape[0], shape[1]
    hw = t[0, 0].numel()
    assert torch.equal(v, t) and v.shape == t.shape and _planes_dense(v)
    want = {"dense": (0, c * hw, hw), "slice": (None, (c + 2) * hw, hw), "off4": (4, c * hw, hw), "off8": (8, c * hw, hw),
            "pad1": (0, c * (hw + 1), hw + 1), "pad2": (0, c * (hw + 2), hw + 2)}[layout]
    if want[0] is not None:
        assert v.data_ptr() % 16 == want[0]
    else:
        assert v.data_ptr() - big.data_ptr() == 4 * hw
    assert (v.stride(0), v.stride(1)) == want[1:]
    # everything of the backing buffer that is not the view is NaN, and the view is exactly t.numel() elements of it
    flat = big.reshape(-1)
    assert int(torch.isnan(flat).sum()) == flat.numel() - t.numel()
    assert big.data_ptr() <= v.data_ptr() and v.data_ptr() + 4 * ((n - 1) * v.stride(0) + (c - 1) * v.stride(1) + hw) <= \
        big.data_ptr() + 4 * flat.numel()
    assert canary_intact(v, big)


def test_the_gates_each_layout_is_meant_for():
    """off8 passes an 8-byte gate and fails a 16-byte one; pad2 passes `& 1` and fails `& 3`; pad1 fails both; off4 fails both"""
    t = _t((2, 3, 4, 8))
    for layout, p8, p16, s1, s3 in [("off4", False, False, True, True), ("off8", True, False, True, True),
                                    ("pad1", True, True, False, False), ("pad2", True, True, True, False)]:
        v, _ = place(t, CPU, layout)
        assert (v.data_ptr() % 8 == 0) == p8 and (v.data_ptr() % 16 == 0) == p16, layout
        assert ((v.stride(0) | v.stride(1)) % 2 == 0) == s1 and ((v.stride(0) | v.stride(1)) % 4 == 0) == s3, layout


@pytest.mark.parametrize("layout", [l for l in LAYOUTS if l != "dense"])
def test_canary_sees_what_a_kernel_can_do_wrong(layout):
    t = _t((2, 3, 4, 8))
    v, big = place(t, CPU, layout)
    v.fill_(float("nan"))                       # a destination before the kernel runs
    assert not canary_intact(v, big)            # nothing written yet
    v.copy_(t)
    assert canary_intact(v, big)
    off = (v.data_ptr() - big.data_ptr()) // 4
    flat = big.reshape(-1)
    # one element past each end of the view, and (strided layouts) the gap between two planes / samples
    outside = [i for i in (off - 1, off + (v.shape[0] - 1) * v.stride(0) + (v.shape[1] - 1) * v.stride(1) + 32,
                           off + 32 if layout in ("pad1", "pad2") else -1,
                           off + v.shape[1] * v.stride(1) if layout == "slice" else -1) if 0 <= i < flat.numel()]
    assert outside
    for i in outside:
        assert torch.isnan(flat[i]), (layout, i)
        flat[i] = 0.0
        assert not canary_intact(v, big), (layout, i)
        flat[i] = float("nan")
        assert canary_intact(v, big)
    v[1, 2, 3, 7] = float("nan")                # an element the kernel did not write
    assert not canary_intact(v, big)
    v[1, 2, 3, 7] = float("inf")                # a non-finite result
    assert not canary_intact(v, big)
    v[1, 2, 3, 7] = 1.0
    assert canary_intact(v, big)


def test_dense_layout_has_no_surroundings():
    t = _t((2, 3, 4, 8))
    v, big = place(t, CPU, "dense")
    assert v.data_ptr() == big.data_ptr() and big.numel() == t.numel() and canary_intact(v, big)
    v[0, 0, 0, 0] = float("nan")
    assert not canary_intact(v, big)


def test_the_pointwise_tests_padded_rows():
    """place_view(..., "pad"): [N,C,L] rows of L + 1 inside a C + 2 channel buffer, as tests/test_pointwise_edges_gpu.py uses it"""
    t = _t((3, 4, 64))
    v = place_view(t, CPU, "pad")
    assert torch.equal(v, t) and v.stride() == (6 * 65, 65, 1)
    with pytest.raises(ValueError):
        place(t, CPU, "no such layout")
