"""CPU: what ``ocrf_bev_pool_v2_nchw_panel_stats`` refuses at the C boundary and that a recorded step can hold it —
argument validation alone, like the host-only checks of tests/test_abi.py (the calls return before anything is launched)."""
import ctypes

from ocrfdet_amd import _lib

INVALID = 1                                       # hipErrorInvalidValue


def _call(L, Z=1, layout=1, stats=True, feat_bytes=1 << 20, c=80):
    p = ctypes.c_void_p(4096)                     # any non-null, 16-byte aligned value: never dereferenced
    return L.ocrf_bev_pool_v2_nchw_panel_stats(c, 4, p, p, p, p, p, p, p, p, p, p, 1, Z, 8, 8, layout, p, p,
                                               ctypes.c_size_t(feat_bytes), p if stats else None, None)


def test_the_entry_point_refuses_planes_rows_layout_and_null_stats():
    L = _lib.lib()
    assert _call(L, Z=2) == INVALID
    assert _call(L, layout=2) == INVALID
    assert _call(L, stats=False) == INVALID
    # the refusals of ocrf_bev_pool_v2_nchw_panel stay
    assert _call(L, feat_bytes=1 << 31) == INVALID and _call(L, c=48) == INVALID and _call(L, layout=3) == INVALID


def test_a_step_can_hold_the_entry_point():
    L = _lib.lib()
    fid = L.ocrf_step_fn_id(b'ocrf_bev_pool_v2_nchw_panel_stats')
    assert fid >= 0 and fid != L.ocrf_step_fn_id(b'ocrf_bev_pool_v2_nchw_panel')
    _, argtypes = _lib.prototypes()['ocrf_bev_pool_v2_nchw_panel_stats']
    _, plain = _lib.prototypes()['ocrf_bev_pool_v2_nchw_panel']
    assert argtypes == plain[:-1] + [ctypes.c_void_p, ctypes.c_void_p]           # ... + float *stats, then the stream
    assert L.ocrf_step_fn_args(fid) == len(argtypes) - 1 == 21
    assert 'ocrf_bev_pool_v2_nchw_panel_stats' in _lib._ENQUEUEING
