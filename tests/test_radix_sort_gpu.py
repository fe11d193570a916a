"""The library's stable LSD radix sort (csrc/radix_sort.hip) on its own, through ocrf_diag_radix_sort: the plain
key / value last pass and every pass count, which neither caller of the sort runs (the LSS preparation sorts in 1-3
passes into the rank vectors, the render-plan build in 4 into the plan's lists).  Sorted keys and ids must equal
numpy's stable argsort exactly: ids ascending among equal keys is the stability both callers rely on."""
import ctypes

import numpy as np
import pytest
import torch

from ocrfdet_amd import _lib

# one ragged chunk | the chunk boundary (2048 keys per workgroup) on both sides | 9 and 20 workgroups = 3 and 5
# look-back tiles of the scan over the 512 x workgroups table
SIZES = [1, 64, 2047, 2048, 2049, 18433, 40000]
KEY_BITS = [1, 9, 10, 18, 19, 27, 28, 32]          # both sides of every step of the pass count (9 bits per pass)
INVALID = 1                                        # hipErrorInvalidValue


def _patterns(n, key_bits, rng):
    """uniform | at most 7 distinct values (long runs of ties) | descending: strictly where 2^key_bits >= n, else as
    evenly as the range allows (a strictly descending sequence of n keys needs n values)."""
    top = 1 << key_bits
    yield 'uniform', rng.integers(0, top, n, dtype=np.uint64).astype(np.uint32)
    values = rng.integers(0, top, 7, dtype=np.uint64).astype(np.uint32)
    yield 'ties', values[rng.integers(0, 7, n)]
    down = (np.arange(n - 1, -1, -1, dtype=np.uint64) * np.uint64(top) // np.uint64(n)).astype(np.uint32)
    assert np.all(np.diff(down.astype(np.int64)) < 0) or top < n
    yield 'descending', down


@pytest.mark.gpu
@pytest.mark.parametrize('key_bits', KEY_BITS)
@pytest.mark.parametrize('n', SIZES)
def test_radix_sort_equals_the_stable_argsort(cuda, n, key_bits):
    L = _lib.lib()
    rng = np.random.default_rng(1000 * key_bits + n)
    ws = torch.empty(int(L.ocrf_diag_radix_sort_workspace_bytes(n)), dtype=torch.uint8, device=cuda)
    off, n_states, stride = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_long(0)
    _lib.check(L.ocrf_diag_radix_sort_states(_lib.ptr(ws), n, key_bits, ctypes.byref(off), ctypes.byref(n_states),
                                             ctypes.byref(stride)), 'ocrf_diag_radix_sort_states')
    assert n_states.value == (key_bits + 8) // 9
    assert off.value % 8 == 0 and off.value + 8 * stride.value * n_states.value <= ws.numel()
    for name, keys in _patterns(n, key_bits, rng):
        assert keys.shape == (n,) and int(keys.max()) < (1 << key_bits)
        dev_keys = torch.from_numpy(keys.view(np.int32)).to(cuda)          # clobbered by the sort
        out_keys = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        out_ids = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        _lib.launch('ocrf_diag_radix_sort', cuda, dev_keys, n, key_bits, out_keys, out_ids, ws, ws.numel())
        order = np.argsort(keys, kind='stable')
        np.testing.assert_array_equal(out_ids.cpu().numpy(), order.astype(np.int32), err_msg=f'{name}: ids')
        np.testing.assert_array_equal(out_keys.cpu().numpy().view(np.uint32), keys[order], err_msg=f'{name}: keys')
        # first word of every pass's look-back state block: bit 63 = that scan gave up
        words = ws[off.value:off.value + 8 * stride.value * n_states.value].view(torch.int64)[::stride.value]
        assert words.numel() == n_states.value and bool((words >= 0).all()), f'{name}: a look-back scan gave up'


def test_radix_sort_refuses_bad_arguments_before_any_launch():
    """Host side only: the pointers are never dereferenced."""
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    n = 5000
    size = L.ocrf_diag_radix_sort_workspace_bytes(n)
    assert size > 3 * 4 * n and L.ocrf_diag_radix_sort_workspace_bytes(0) == 0
    assert L.ocrf_diag_radix_sort(p, 0, 32, p, p, p, ctypes.c_size_t(size), None) == INVALID
    for key_bits in (0, 33):
        assert L.ocrf_diag_radix_sort(p, n, key_bits, p, p, p, ctypes.c_size_t(size), None) == INVALID
    assert L.ocrf_diag_radix_sort(p, n, 32, p, p, p, ctypes.c_size_t(size - 1), None) == INVALID
