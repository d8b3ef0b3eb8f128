"""Memory layouts a kernel can be handed behind the [N,C,...] ABI (any pointer, any sample / channel stride, dense planes),
and the check that a kernel wrote nothing but its own view.

``place(t, dev, layout)`` puts a float32 tensor on ``dev`` as a view of a larger NaN-filled buffer and returns
``(view, backing)``: whatever a kernel reads outside the view is NaN, whatever it writes outside the view overwrites one.

  dense    a buffer of its own
  slice    big[:, 1:C+1] of a tensor with C + 2 channels: sample stride (C+2)*HW, the base HW floats into the buffer
  off4     base pointer = 4 (mod 16), dense strides
  off8     base pointer = 8 (mod 16), dense strides: passes the 8-byte gates, fails the 16-byte ones
  pad1     plane stride HW + 1, sample stride C*(HW+1): odd for planes of 4k elements, fails the `& 1` and `& 3` gates
  pad2     plane stride HW + 2: for planes of 4k elements it passes the `& 1` gates and fails the `& 3` ones
  pad      [N,C,L] only: big[:, 1:C+1, :L] of a buffer with C + 2 channels and rows of L + 1 (the pointwise tests' layout)

Every layout asserts the pointer and stride residues it promises, so a test that names one gets it."""
import torch

LAYOUTS = ("dense", "slice", "off4", "off8", "pad1", "pad2")
NAN = float("nan")


def _hw(t):
    hw = 1
    for d in t.shape[2:]:
        hw *= d
    return hw


def _aligned_flat(numel, lead, dev):
    """a NaN-filled flat buffer and a view of ``numel`` floats that starts ``lead`` floats past a 16-byte boundary"""
    big = torch.full((numel + lead + 4,), NAN, dtype=torch.float32, device=dev)
    skip = (-(big.data_ptr() // 4)) % 4            # (allocators align to far more than 16 bytes; a CPU tensor may not)
    return big[skip + lead: skip + lead + numel], big


def place(t, dev, layout="dense"):
    """(view, backing): ``t`` (float32, [N,C,...]) on ``dev`` in the named layout, surrounded by NaN"""
    assert t.dtype == torch.float32 and t.dim() >= 3, (t.dtype, tuple(t.shape))
    n, c, hw = t.shape[0], t.shape[1], _hw(t)
    if layout == "dense":
        big = torch.full(tuple(t.shape), NAN, dtype=torch.float32, device=dev)
        v = big
        assert v.is_contiguous()
    elif layout == "slice":
        big = torch.full((n, c + 2) + tuple(t.shape[2:]), NAN, dtype=torch.float32, device=dev)
        v = big[:, 1:c + 1]
        assert v.stride(0) == (c + 2) * hw and v.stride(1) == hw and v.data_ptr() - big.data_ptr() == 4 * hw
    elif layout in ("off4", "off8"):
        lead = 1 if layout == "off4" else 2
        flat, big = _aligned_flat(t.numel(), lead, dev)
        v = flat.view(t.shape)
        assert v.data_ptr() % 16 == 4 * lead and v.is_contiguous()
    elif layout in ("pad1", "pad2"):
        extra = 1 if layout == "pad1" else 2
        flat, big = _aligned_flat(n * c * (hw + extra), 0, dev)
        # ([N, C, HW + extra][:, :, :HW] viewed as t.shape; as_strided so that a dimension of size 1 keeps the stride too)
        dense = [1] * (t.dim() - 2)
        for d in range(t.dim() - 4, -1, -1):
            dense[d] = dense[d + 1] * t.shape[d + 3]
        v = torch.as_strided(flat, tuple(t.shape), (c * (hw + extra), hw + extra) + tuple(dense))
        assert v.data_ptr() % 16 == 0 and v.stride(1) == hw + extra and v.stride(0) == c * (hw + extra)
        assert hw % 4 or v.stride(1) % 4 == extra        # (planes of 4k elements: the residue the `& 1` / `& 3` gates see)
    elif layout == "pad":
        assert t.dim() == 3
        big = torch.full((n, c + 2, t.shape[2] + 1), NAN, dtype=torch.float32, device=dev)
        v = big[:, 1:c + 1, :t.shape[2]]
        assert v.stride(1) == t.shape[2] + 1
    else:
        raise ValueError("unknown layout %r" % (layout,))
    assert v.shape == t.shape
    v.copy_(t.to(dev))
    return v, big


def place_view(t, dev, layout="dense"):
    """the view alone (sources, whose surroundings nobody looks at afterwards)"""
    return place(t, dev, layout)[0]


def _view_mask(view, backing):
    """True where ``backing`` (flat) belongs to ``view``: found by writing through the view into a scratch copy's twin"""
    off = (view.data_ptr() - backing.data_ptr()) // 4
    mask = torch.zeros(backing.numel(), dtype=torch.bool, device=backing.device)
    torch.as_strided(mask, tuple(view.shape), view.stride(), off).fill_(True)
    return mask


def canary_intact(view, backing):
    """after a kernel wrote ``view``: every element of ``backing`` outside the view is still NaN and the view is finite"""
    assert view.dtype == torch.float32 and backing.dtype == torch.float32 and backing.is_contiguous()
    mask = _view_mask(view, backing)
    flat = backing.reshape(-1)
    outside_ok = bool(torch.isnan(flat[~mask]).all())
    inside_ok = bool(torch.isfinite(flat[mask]).all())
    return outside_ok and inside_ok
