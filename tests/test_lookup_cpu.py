"""Prompt-lookup drafting without a GPU: the yardstick of the GPU tests (test_gpu_lookup_ops.ngram_rule) against a brute-force restatement, the two C-ABI
names in header and binding, and the refusal to run without a device."""
import numpy as np

from test_cabi_exports import declared_symbols
from test_gpu_lookup_ops import ngram_rule


def brute(h, ngram_min, ngram_max, k):
    """every (m, e) by comparing whole slices, then the largest pair"""
    n = len(h)
    pairs = [(next(m for m in range(min(ngram_max, e), -1, -1) if h[e - m:e] == h[n - m:n]), e) for e in range(1, n)]
    m, e = max(pairs) if pairs else (0, 0)
    return (h[e:e + k] if m >= ngram_min else []), m, e


def test_rule_equals_brute_force():
    rng = np.random.default_rng(0)
    for _ in range(400):
        h = rng.integers(0, int(rng.integers(1, 5)), int(rng.integers(0, 40))).tolist()
        ngram_max = int(rng.integers(1, 17))
        args = (int(rng.integers(1, ngram_max + 1)), ngram_max, int(rng.integers(1, 17)))
        assert ngram_rule(h, *args) == brute(h, *args), (h, args)


def test_symbols_are_declared_and_answer_no_device(pkg):
    for name in ("mi355_op_ngram_draft", "mi355_lookup_steps"):
        assert name in declared_symbols() and name in pkg.binding.SYMBOLS
    lib = pkg.load_library()
    out = np.zeros(16, np.int32)
    rc = lib.mi355_lookup_steps(None, out.ctypes.data, 4, 1, 4, 0, 1, 2, 4, 16, 0, out.ctypes.data, None)
    assert rc < 0 and lib.mi355_last_error()
    if lib.mi355_device_count() == 0:                                      # the device is asked for before the context or any argument is looked at
        assert rc == -100
        assert lib.mi355_op_ngram_draft(out.ctypes.data, 1, 16, out.ctypes.data, 2, 4, 8, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -100
