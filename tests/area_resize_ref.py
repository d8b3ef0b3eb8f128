"""Shared by tests/test_area_resize.py and tests/test_area_resize_gpu.py: the restatements of scripts/make_area_resize_golden.py
(loaded from its file), the two fixture files, and bit-for-bit comparison."""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_area_resize_golden")
GOLD = np.load(G.PATH)
EDGES = json.load(open(G.EDGES))


def same_bits(a, b):
    """a device tensor or array against an array: dtype, shape and every bit"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                        np.ascontiguousarray(b).view(np.uint8))
