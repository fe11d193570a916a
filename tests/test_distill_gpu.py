"""GPU: the fused correlation volume (``ocrf_group_corr_forward`` / ``_backward``) and the fused distillation losses
(``ocrf_kd_losses_forward`` / ``_backward``) against the float64 oracle of ``tests/distill_oracle.py`` with its derived
bounds, their launch counts, reruns, refusals and strides, and ``OcRFDet4DVGGT`` with and without the kernels."""
import ctypes
import random

import numpy as np
import pytest
import torch
from torch import nn

from ocrfdet_amd import _lib, distill

from tests import distill_oracle as oracle
from tests import test_distill_host as host

pytestmark = pytest.mark.gpu

# (B, C, H, W, G, D): W = 1 (everything clamps); W < D with Cg = 2; Cg = 1 and D = 1; a row of exactly one wave and one
# past it with Cg = 3; the config's plane of 777 pixels (four chunks, the last one partial) with Cg = 1; Cg = 32 (four
# staging steps); the largest D (the second kernel instantiation)
SMALL = [(1, 4, 1, 1, 1, 5), (2, 6, 2, 3, 3, 5), (1, 7, 3, 5, 7, 1), (2, 12, 3, 64, 4, 5), (1, 12, 2, 65, 4, 5),
         (1, 64, 21, 37, 64, 5), (2, 96, 21, 37, 3, 5), (1, 8, 4, 40, 2, 16)]
FULL = (2, 2048, 21, 37, 64, 5)                   # the config's features
KD_FULL = (4, 248640)                             # the config's volumes at samples_per_gpu = 4


def operands(cuda, shape, integers=False):
    b, c, h, w, g, d = shape
    gen = torch.Generator().manual_seed(sum(shape) + 13 * integers)
    if integers:
        feats = torch.randint(-3, 4, (b, 2, c, h, w), generator=gen).float()
        grad_out = torch.randint(-2, 3, (b, g, d, h, w), generator=gen).float()
    else:
        feats = torch.randn(b, 2, c, h, w, generator=gen)
        grad_out = torch.randn(b, g, d, h, w, generator=gen)
    return feats.to(cuda).requires_grad_(True), grad_out.to(cuda)


def run(feats, grad_out, shape):
    g, d = shape[4:]
    feats.grad = None
    out = distill.build_cost_volume(feats, max_disp=d - 1, method='group_corr', groups=g, fused=True)
    out.backward(grad_out)
    return out.detach(), feats.grad


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('shape', SMALL)
def test_volume_and_gradients_match_the_oracle(cuda, shape):
    b, c, h, w, g, d = shape
    feats, grad_out = operands(cuda, shape)
    out, grad = run(feats, grad_out, shape)
    assert out.shape == (b, g, d, h, w) and out.is_contiguous() and grad.shape == feats.shape
    left, right = feats.detach()[:, 0].cpu().numpy(), feats.detach()[:, 1].cpu().numpy()
    want, n, mag = oracle.volume(left, right, g, d)
    err = np.abs(out.cpu().numpy() - want)
    print(f'{shape}: volume max err {err.max():.3e}, bound there {oracle.sum_bound(n, mag).flat[err.argmax()]:.3e}')
    assert (err <= oracle.sum_bound(n, mag)).all()
    gL, nL, magL, gR, nR, magR = oracle.volume_grads(left, right, grad_out.cpu().numpy(), g, d)
    grad = grad.cpu().numpy()
    errL, errR = np.abs(grad[:, 0] - gL), np.abs(grad[:, 1] - gR)
    print(f'{shape}: gL max err {errL.max():.3e}, gR max err {errR.max():.3e} (column 0: {errR[..., 0].max():.3e})')
    assert (errL <= oracle.sum_bound(nL, magL)).all()
    assert (errR <= oracle.sum_bound(nR, magR)).all()


def test_integer_valued_inputs_are_exact(cuda):
    """Every product and partial sum is an integer far below 2^24: float32 sums are exact in any order."""
    shape = (2, 12, 3, 64, 4, 5)
    b, c, h, w, g, d = shape
    feats, grad_out = operands(cuda, shape, integers=True)
    out, grad = run(feats, grad_out, shape)
    left, right = feats.detach()[:, 0].cpu().numpy(), feats.detach()[:, 1].cpu().numpy()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), oracle.volume(left, right, g, d)[0])
    gL, _, _, gR, _, _ = oracle.volume_grads(left, right, grad_out.cpu().numpy(), g, d)
    assert np.array_equal(grad[:, 0].cpu().numpy().astype(np.float64), gL)
    assert np.array_equal(grad[:, 1].cpu().numpy().astype(np.float64), gR)


@pytest.fixture(scope='module')
def full(cuda):
    """The full-size case, run once: operands, the kernels' results and the oracle's (the whole volume; the gradients of
    three groups' channels, every pixel of them, column 0 included)."""
    b, c, h, w, g, d = FULL
    feats, grad_out = operands(cuda, FULL)
    out, grad = run(feats, grad_out, FULL)
    f = feats.detach().cpu().numpy()
    want, n, mag = oracle.volume(f[:, 0], f[:, 1], g, d)
    groups = [0, 31, 63]
    cg = c // g
    channels = np.concatenate([np.arange(k * cg, (k + 1) * cg) for k in groups])
    grads = oracle.volume_grads(f[:, 0][:, channels], f[:, 1][:, channels], grad_out.cpu().numpy()[:, groups], len(groups), d)
    return dict(feats=feats, grad_out=grad_out, out=out, grad=grad, want=(want, n, mag), channels=channels, grads=grads)


def test_full_size_volume_and_sampled_gradients(full):
    want, n, mag = full['want']
    err = np.abs(full['out'].cpu().numpy() - want)
    print(f'{FULL}: volume max err {err.max():.3e}, max |value| {np.abs(want).max():.3f}')
    assert (err <= oracle.sum_bound(n, mag)).all()
    gL, nL, magL, gR, nR, magR = full['grads']
    grad = full['grad'].cpu().numpy()[:, :, full['channels']]
    errL, errR = np.abs(grad[:, 0] - gL), np.abs(grad[:, 1] - gR)
    print(f'{FULL}: gL max err {errL.max():.3e}, gR max err {errR.max():.3e} (column 0: {errR[..., 0].max():.3e})')
    assert (errL <= oracle.sum_bound(nL, magL)).all()
    assert (errR <= oracle.sum_bound(nR, magR)).all()
    assert nR[0] == 15 and (errR[..., 0] <= oracle.sum_bound(nR, magR)[..., 0]).all()


def test_views_of_one_tensor_equal_fresh_copies(cuda):
    """The halves of a (B, 2, C, H, W) tensor are read in place, through the batch stride."""
    shape = (2, 12, 3, 65, 4, 5)
    feats, _ = operands(cuda, shape)
    feats = feats.detach()
    in_place = distill.corr_forward_views(feats[:, 0], feats[:, 1], 4, 5)
    left, right = feats[:, 0].contiguous(), feats[:, 1].contiguous()
    assert left.data_ptr() != feats.data_ptr() and left.stride(0) * 2 == feats.stride(0)
    assert same_bits(in_place, distill.corr_forward_views(left, right, 4, 5))
    assert same_bits(in_place, distill.build_cost_volume(feats, max_disp=4, method='group_corr', groups=4, fused=True))
    # the torch formulation on the device, to the oracle's bound of each
    want, n, mag = oracle.volume(left.cpu().numpy(), right.cpu().numpy(), 4, 5)
    torch_out = distill.build_cost_volume(feats, max_disp=4, method='group_corr', groups=4, fused=False)
    assert (np.abs(torch_out.cpu().numpy() - want) <= oracle.sum_bound(n, mag)).all()


# ------------------------------------------------------------------------------------------------ the two losses
def kd_run(s, t, g_smooth, g_cos):
    s = s.detach().requires_grad_(True)
    smooth, cos = distill.kd_losses(s, t, fused=True)
    grad, = torch.autograd.grad([smooth, cos], [s], [g_smooth, g_cos])
    return smooth.detach(), cos.detach(), grad


@pytest.fixture(scope='module')
def kd_full(cuda):
    s, t = host.kd_operands(*KD_FULL, seed=77)
    gs, gc = torch.tensor(0.75, device=cuda), torch.tensor(-1.5, device=cuda)
    got = kd_run(s.to(cuda), t.to(cuda), gs, gc)
    return dict(s=s, t=t, gs=gs, gc=gc, got=got)


def check_kd(s, t, got, g_smooth=0.75, g_cos=-1.5):
    smooth, cos, grad = got
    want = oracle.kd_losses(s.numpy(), t.numpy())
    print(f'{tuple(s.shape)}: smooth {smooth.item():.9g} (oracle {want[0]:.9g}), cos {cos.item():.9g} (oracle {want[1]:.9g})')
    assert smooth.dim() == 0 and cos.dim() == 0 and smooth.dtype == cos.dtype == torch.float32
    assert abs(smooth.item() - want[0]) <= oracle.loss_bound(want[0])
    assert abs(cos.item() - want[1]) <= oracle.loss_bound(want[1])
    want_grad, mag = oracle.kd_grad(s.numpy(), t.numpy(), g_smooth, g_cos)
    err = np.abs(grad.cpu().numpy() - want_grad)
    assert np.isfinite(grad.cpu().numpy()).all()
    assert (err <= oracle.grad_bound(mag) + 1e-30).all()


@pytest.mark.parametrize('b, n', [(1, 1), (3, 40), (2, 255), (2, 257)])
def test_losses_and_gradient_match_the_oracle(cuda, b, n):
    s, t = host.kd_operands(b, n, seed=10 * b + n)
    if b == 3:
        s[1] = 0.0
    gs, gc = torch.tensor(0.75, device=cuda), torch.tensor(-1.5, device=cuda)
    check_kd(s, t, kd_run(s.to(cuda), t.to(cuda), gs, gc))


def test_losses_at_the_full_size(kd_full):
    check_kd(kd_full['s'], kd_full['t'], kd_full['got'])


def test_equal_volumes_have_no_loss(cuda):
    v = torch.randn(2, 4, 5, 3, 7, generator=torch.Generator().manual_seed(5)).to(cuda)
    smooth, cos = distill.kd_losses(v, v.clone(), fused=True)
    assert smooth.item() == 0.0 and abs(cos.item()) <= oracle.loss_bound(0.0)
    # volumes of any rank are flattened per sample; the teacher gets no gradient
    s, t = v.clone().requires_grad_(True), (v + 0.5).requires_grad_(True)
    sum(distill.kd_losses(s, t, fused=True)).backward()
    assert s.grad is not None and t.grad is None


# ------------------------------------------------------------------------------------------------ structure
def test_reruns_are_bit_identical(cuda, full, kd_full):
    out, grad = run(full['feats'], full['grad_out'], FULL)
    assert same_bits(out, full['out']) and same_bits(grad, full['grad'])
    again = kd_run(kd_full['s'].to(cuda), kd_full['t'].to(cuda), kd_full['gs'], kd_full['gc'])
    assert all(same_bits(a.view(-1), b.view(-1)) for a, b in zip(again, kd_full['got']))
    shape = (2, 6, 2, 3, 3, 5)
    feats, grad_out = operands(cuda, shape)
    first = [t.clone() for t in run(feats, grad_out, shape)]
    assert all(same_bits(a, b) for a, b in zip(first, run(feats, grad_out, shape)))
    s, t = host.kd_operands(3, 40, seed=1)
    gs, gc = torch.tensor(1.0, device=cuda), torch.tensor(1.0, device=cuda)
    first = kd_run(s.to(cuda), t.to(cuda), gs, gc)
    assert all(same_bits(a.view(-1), b.view(-1)) for a, b in zip(first, kd_run(s.to(cuda), t.to(cuda), gs, gc)))


def test_launch_counts_and_no_synchronisation(cuda):
    """Forward of a volume: one launch; its backward: two; the losses: two forward, one backward; none of them reads
    anything back (torch's sync debug mode raises on a synchronising call)."""
    from torch.profiler import ProfilerActivity, profile
    shape = (2, 96, 21, 37, 3, 5)
    feats, grad_out = operands(cuda, shape)
    s, t = (x.to(cuda) for x in host.kd_operands(2, 257, seed=3))
    s.requires_grad_(True)
    gs, gc = torch.tensor(0.75, device=cuda), torch.tensor(-1.5, device=cuda)
    run(feats, grad_out, shape)                                  # warm-up: the library, the scratch buffer
    kd_run(s, t, gs, gc)
    feats.grad = None                                            # the backward then stores its result, it adds nothing
    torch.cuda.synchronize()

    def kernels(fn):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            result = fn()
        names = sorted(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return result, names

    def are(names, *parts):
        return len(names) == len(parts) and all(any(part in n for n in names) for part in parts)
    torch.cuda.set_sync_debug_mode('error')
    try:
        out, names = kernels(lambda: distill.build_cost_volume(feats, max_disp=4, method='group_corr', groups=3))
        assert are(names, 'group_corr_forward_kernel'), names
        _, names = kernels(lambda: out.backward(grad_out))
        assert are(names, 'group_corr_grad_left_kernel', 'group_corr_grad_right_kernel'), names
        losses, names = kernels(lambda: distill.kd_losses(s, t))
        assert are(names, 'kd_partial_kernel', 'kd_final_kernel'), names
        _, names = kernels(lambda: torch.autograd.grad(list(losses), [s], [gs, gc]))
        assert are(names, 'kd_backward_kernel'), names
    finally:
        torch.cuda.set_sync_debug_mode('default')


def test_entry_points_refuse_bad_arguments_and_touch_nothing(cuda):
    L = _lib.lib()
    invalid = 1                                                  # hipErrorInvalidValue
    b, c, h, w, g, d = 2, 12, 3, 7, 4, 5
    feats = torch.randn(b, 2, c, h, w, device=cuda)
    out = torch.full((b, g, 17, h, w), 7.0, device=cuda)         # room for every D tried
    grad = torch.full_like(feats, 7.0)
    grad_out = torch.randn(b, g, 17, h, w, device=cuda)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    left, right, stride = p(feats), p(feats[:, 1]), 2 * c * h * w
    stream = _lib.stream_ptr(cuda)

    def forward(c=c, g=g, d=d, left=left, out=p(out), stride=stride):
        return L.ocrf_group_corr_forward(b, c, h, w, g, d, left, right, stride, out, stream)

    def backward(c=c, g=g, d=d, left=left, grad_left=p(grad)):
        return L.ocrf_group_corr_backward(b, c, h, w, g, d, p(grad_out), left, right, stride, grad_left, p(grad[:, 1]),
                                          stride, stream)
    for fn in (forward, backward):
        assert fn(g=5) == invalid and fn(d=0) == invalid and fn(d=17) == invalid and fn(left=None) == invalid
    assert forward(out=None) == invalid and backward(grad_left=None) == invalid
    assert forward(stride=c * h * w - 1) == invalid              # samples would overlap
    s, t = torch.randn(2, 40, device=cuda), torch.randn(2, 40, device=cuda)
    losses, sums = torch.full((2,), 7.0, device=cuda), torch.full((2, 3), 7.0, device=cuda, dtype=torch.float64)
    nbytes = L.ocrf_kd_losses_workspace_bytes(2, 40)
    assert nbytes > 0 and L.ocrf_kd_losses_workspace_bytes(0, 40) == 0 and L.ocrf_kd_losses_workspace_bytes(2, 1 << 31) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    grad_s = torch.full_like(s, 7.0)
    size = ctypes.c_size_t(nbytes)
    assert L.ocrf_kd_losses_forward(2, 40, None, p(t), p(losses), p(losses[1:]), p(sums), p(ws), size, stream) == invalid
    assert L.ocrf_kd_losses_forward(2, 40, p(s), p(t), p(losses), p(losses[1:]), p(sums), None, size, stream) == invalid
    assert L.ocrf_kd_losses_forward(2, 40, p(s), p(t), p(losses), p(losses[1:]), p(sums), p(ws),
                                    ctypes.c_size_t(nbytes - 1), stream) == invalid
    assert L.ocrf_kd_losses_forward(0, 40, p(s), p(t), p(losses), p(losses[1:]), p(sums), p(ws), size, stream) == invalid
    assert L.ocrf_kd_losses_backward(2, 40, p(s), p(t), None, p(losses), p(losses[1:]), p(grad_s), stream) == invalid
    assert L.ocrf_kd_losses_backward(2, 0, p(s), p(t), p(sums), p(losses), p(losses[1:]), p(grad_s), stream) == invalid
    torch.cuda.synchronize()
    for buf in (out, grad, losses, sums, grad_s):
        assert bool((buf == 7.0).all())
    # the Python layer refuses before any call
    half = feats.detach().half()
    for bad in (half, feats.cpu(), feats.transpose(3, 4), feats.double()):
        with pytest.raises(_lib.OcrfHipError):
            distill.build_cost_volume(bad, max_disp=4, method='group_corr', groups=4, fused=True)
    with pytest.raises(_lib.OcrfHipError):
        distill.build_cost_volume(feats, max_disp=16, method='group_corr', groups=4, fused=True)
    with pytest.raises(_lib.OcrfHipError):
        distill.kd_losses(s.double(), t.double(), fused=True)
    with pytest.raises(_lib.OcrfHipError):
        distill.kd_losses(s.t(), t.t(), fused=True)
    # ... and without the request for the kernels, the same operands take the torch formulation
    assert distill.build_cost_volume(feats.transpose(3, 4), max_disp=4, method='group_corr', groups=4).shape == (b, g, 5, w, h)


def test_autocast_runs_the_kernels_in_float32(cuda):
    shape = (2, 12, 3, 9, 4, 5)
    feats, _ = operands(cuda, shape)
    feats = feats.detach()
    want = distill.build_cost_volume(feats.bfloat16().float(), max_disp=4, method='group_corr', groups=4, fused=True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        got = distill.build_cost_volume(feats.bfloat16(), max_disp=4, method='group_corr', groups=4)
        full = distill.build_cost_volume(feats, max_disp=4, method='group_corr', groups=4)
        losses = distill.kd_losses(got, full)
    assert got.dtype == torch.float32 and same_bits(got, want)
    assert same_bits(full, distill.build_cost_volume(feats, max_disp=4, method='group_corr', groups=4, fused=True))
    assert all(v.dtype == torch.float32 for v in losses)


# ------------------------------------------------------------------------------------------------ the detector
class DeviceViewTransformer(nn.Module):
    """The least a view transformer must return, on whatever device its input lies: the distillation branch does not
    read it."""
    downsample = 16

    def __init__(self):
        super().__init__()
        self.grid_config = dict(depth=[1.0, 60.0, 0.5])
        self.cv_frustum = torch.zeros(2, 2, 2, 3)

    def forward(self, inputs, metas):
        x = inputs[0]
        bev = x.reshape(x.shape[0], -1)[:, :32].view(-1, 2, 4, 4)
        return bev, torch.sigmoid(bev[:, :1]), (bev[:, 1:], torch.sigmoid(bev)), [bev, None, None, None, None, None, None,
                                                                                None, None]


def test_detector_with_and_without_the_kernels(cuda):
    det = host.vggt_detector(host.StandInAggregator(), vt=DeviceViewTransformer()).to(cuda).train()
    inputs = [t.to(cuda) for t in host.GS.make_inputs(n=host.N)]
    results = {}
    for fused in (True, False):
        det.fused_distill = fused
        det.zero_grad(set_to_none=True)
        random.seed(9)
        volume_t, volume_s = det.extract_img_feat(inputs, None)[4]
        losses = distill.kd_losses(volume_s, volume_t, fused=fused)
        sum(losses).backward()
        results[fused] = ([v.item() for v in losses], {k: p.grad.clone() for k, p in det.aligner.named_parameters()})
    (fused_losses, fused_grads), (torch_losses, torch_grads) = results[True], results[False]
    for a, b in zip(fused_losses, torch_losses):
        print(f'fused {a:.9g} torch {b:.9g}')
        assert abs(a - b) <= oracle.loss_bound(b)
    for k in fused_grads:
        # a bias of the keys moves every logit of a softmax row alike: its gradient is zero in exact arithmetic, rounding
        # noise (1e-10) in both arms, and has no magnitude of its own; it is held to the scale of the key weights' gradient
        scale = torch_grads['key_proj.weight' if k == 'key_proj.bias' else k].abs().max().item()
        assert scale > 0 and (fused_grads[k] - torch_grads[k]).abs().max().item() <= 1e-5 * scale, k
    assert all(p.grad is None for p in det.img_backbone.parameters())
