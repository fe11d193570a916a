"""Host side of HOA-1's fused training path (no library launch): the oracle's inputs, the masked torch fallback, the
autograd Function's contract, the C prototypes and the workspace query."""
import ctypes

import pytest
import torch

from ocrfdet_amd import _lib, hoa
from tests import hoa1_train_oracle as O


@pytest.mark.parametrize('shape', list(O.CASES))
def test_ambiguous_sets_of_the_gpu_tests_inputs_are_empty(shape):
    for masked in (False, True):
        ref = O.oracle(shape, masked)
        assert ref['ambiguous'] == 0 and ref['touched'] > 0
        assert len(ref['grads']) == 16 and all(torch.isfinite(g).all() for g in ref['grads'])
    assert O.search_seed(shape) == O.CASES[shape]


def test_inputs_cover_samples_inside_and_outside_the_map():
    assert any(O.oracle(s, False)['inside'] > 0 and O.oracle(s, False)['outside'] > 0 for s in O.CASES)


def test_masked_fallback_has_dropout_semantics():
    """The mask multiplies ``attn`` after the softmax, with the scale 1 / (1 - p) — what nn.Dropout does with the same
    keep decisions — whatever the module's mode; all ones with p = 0 is no dropout."""
    shape = (2, 36, 60)
    m = O.make_module()
    op, al, _, mask = O.make_inputs(shape)
    hq, wq, _, _ = O.token_counts(*shape[1:])
    o_up = torch.nn.functional.interpolate(op, size=(hq, wq), mode='bilinear', align_corners=True)
    a_up = torch.nn.functional.interpolate(al, size=(hq, wq), mode='bilinear', align_corners=True)
    seen = {}
    real_dropout = m.dropout

    class Spy(torch.nn.Module):                 # nn.Dropout's keep decisions replaced by the mask's: attn in, scaled out
        p = real_dropout.p

        def forward(self, attn):
            seen['attn'] = attn
            return attn * mask.unsqueeze(1) / (1.0 - self.p)
    with torch.no_grad():
        m.dropout = Spy()
        want = m(o_up, a_up)
        m.dropout = real_dropout
        assert torch.allclose(seen['attn'].sum(-1), torch.ones(()), atol=1e-6)         # after the softmax
        for mode in (m.train, m.eval):
            mode()
            torch.testing.assert_close(m(o_up, a_up, dropout_mask=mask), want, rtol=1e-6, atol=1e-7)
            full = hoa.hoa1(m, op.reshape(-1, 1), al, 13, *shape[1:], dropout_mask=mask)
            up = torch.nn.functional.interpolate(want, size=shape[1:], mode='bilinear', align_corners=True) + op
            torch.testing.assert_close(full, up, rtol=1e-6, atol=1e-7)
        m.eval()
        m.dropout.p = 0.0
        assert torch.equal(m(o_up, a_up, dropout_mask=torch.ones_like(mask)), m(o_up, a_up))
    assert hoa._dropout_scale(0.1) == pytest.approx(1 / 0.9) and hoa._dropout_scale(0.0) == 1.0


def test_switch_off_leaves_the_dispatch_as_it_was():
    """``fused_training`` defaults to False; a module in train(), or anything that requires grad, still takes the torch
    sequence (``_hoa1_fusable`` unchanged), and so does a CPU tensor with the switch on."""
    import inspect
    sig = inspect.signature(hoa.hoa1)
    assert sig.parameters['fused_training'].default is False and sig.parameters['dropout_mask'].default is None
    from ocrfdet_amd import view_transformer_ocrf as vto
    assert vto.OcRFViewTransformerFull.fused_hoa1_training is False

    class FakeCuda:
        is_cuda, requires_grad = True, False
    m = O.make_module()
    with torch.no_grad():
        assert hoa._hoa1_fusable(m, FakeCuda())
        assert not hoa._hoa1_fusable(m.train(), FakeCuda())
    m.eval()
    assert not hoa._hoa1_fusable(m, FakeCuda())                    # grad enabled, parameters require grad
    op, al, _, _ = O.make_inputs((2, 36, 36))
    o = op.clone().requires_grad_(True)
    on = hoa.hoa1(m, o.reshape(-1, 1), al, 13, 36, 36, fused_training=True)
    assert type(on.grad_fn).__name__ != '_Hoa1TrainBackward'
    assert torch.equal(on, hoa.hoa1(m, o.reshape(-1, 1), al, 13, 36, 36))


def test_function_contract_without_a_launch(monkeypatch):
    """The Function packs once, hands the library the workspace it asked it for, returns the 14 parameter gradients as
    views of ONE packed vector, and refuses a double backward."""
    calls = []

    def fake_launch(name, device, *args, stream=None):
        calls.append((name, args))
        if name == 'ocrf_hoa1_forward_train':
            args[-1].copy_(args[0])
        else:
            for t in args[-3:]:
                t.fill_(1.0)
    monkeypatch.setattr(_lib, 'launch', fake_launch)
    m = O.make_module()
    shape = (2, 36, 60)
    op, al, go, mask = O.make_inputs(shape)
    o, a = op.clone().requires_grad_(True), al.clone().requires_grad_(True)
    params = hoa._hoa1_params(m)
    out = hoa._Hoa1Train.apply(o, a, *params, mask, m, 1.0 / 0.9)
    assert type(out.grad_fn).__name__ == '_Hoa1TrainBackward'
    name, args = calls[0]
    L = _lib.lib()
    assert name == 'ocrf_hoa1_forward_train' and args[-2].numel() == L.ocrf_hoa1_train_workspace_floats(*shape) > 0
    assert args[2].numel() == L.ocrf_hoa1_weights_len() == sum(p.numel() for p in params)
    assert args[2] is hoa._hoa1_packed(m)                          # the cached pack: versions and pointers match
    go.requires_grad_(True)
    grads = torch.autograd.grad(out, [o, a] + params, go, create_graph=True)
    assert calls[1][0] == 'ocrf_hoa1_backward' and calls[1][1][-4].data_ptr() == args[-2].data_ptr()    # the forward's workspace
    assert [g.shape for g in grads[2:]] == [p.shape for p in params]
    base = grads[2]._base if grads[2]._base is not None else grads[2]
    ptr, at = base.data_ptr(), 0
    for g in grads[2:]:                                            # consecutive views of one vector
        assert g.data_ptr() == ptr + 4 * at
        at += g.numel()
    with pytest.raises(RuntimeError, match='once_differentiable|twice'):
        grads[0].sum().backward()


def test_prototypes_kernel_ids_and_workspace_query():
    protos = _lib.prototypes()
    for name, n_args in (('ocrf_hoa1_forward_train', 12), ('ocrf_hoa1_backward', 15)):
        restype, argtypes = protos[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args and argtypes[-1] is ctypes.c_void_p
        assert name in _lib._ENQUEUEING
    restype, argtypes = protos['ocrf_hoa1_train_workspace_floats']
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int] * 3
    assert 'ocrf_hoa1_train_workspace_floats' not in _lib._ENQUEUEING              # host only: no stream
    assert _lib.K_HOA1_KV == 29 and _lib.K_HOA1_ATTN == 26
    L = _lib.lib()
    ids = [_lib.K_HOA1_ATTN_TRAIN, _lib.K_HOA1_UP_GRAD, _lib.K_HOA1_ATTN_GRAD, _lib.K_HOA1_KV_GRAD, _lib.K_HOA1_TOKEN_GRAD,
           _lib.K_HOA1_PIXEL_GRAD, _lib.K_HOA1_WEIGHT_SUM]
    assert ids == list(range(148, 155))
    assert [L.ocrf_kernel_name(i) for i in ids] == [
        b'hoa1_attention_train_kernel', b'hoa1_up_grad_kernel', b'hoa1_attn_grad_kernel', b'hoa1_kv_grad_kernel',
        b'hoa1_token_grad_kernel', b'hoa1_pixel_grad_kernel', b'hoa1_weight_sum_kernel']
    # host only, 0 outside the limits: Y/6 >= 6, X/6 >= 6, <= 1600 query tokens, <= 128 kv tokens
    f = L.ocrf_hoa1_train_workspace_floats
    assert f(2, 36, 36) > 0 and f(2, 128, 128) > f(1, 128, 128) > 0 and f(1, 200, 200) > 0 and f(1, 240, 240) > 0
    assert f(1, 35, 36) == 0 and f(1, 36, 30) == 0 and f(1, 246, 240) == 0 and f(0, 36, 36) == 0
    assert f(1, 36, 1596) > 0 and f(1, 36, 1608) == 0              # 6 x 266 = 1596 tokens, 6 x 268 = 1608
