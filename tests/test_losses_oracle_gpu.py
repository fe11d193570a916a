"""GPU: the fused neck losses of csrc/losses.hip (``depth_labels``, ``depth_semantic_loss``, ``render_losses``,
``ssim``) on the cases of tests/losses_oracle.py, through its checker: depth labels bit for bit against
``depth_labels_torch`` in float32 on the CPU; every loss and every gradient against the float64 evaluation of the
``*_torch`` formulation, within ``max(2 e_torch, floor)`` (see losses_oracle.py), exactly 0 where the oracle is exactly
0.  test_losses_oracle_host.py shows that the cases hit the edges they name and that this bar rejects wrong
formulations.

Measured on an MI355X (worst over the cases of each group, in units of the quantity's floor; torch is the float32
``*_torch`` formulation on the CPU):

    group              quantity        torch    fused
    depth / semantic   loss_depth      0.008    0.009   (floor 1e-5 relative: both are rounding of the sums)
    depth / semantic   loss_sem        0.011    0.011
    depth / semantic   g_depth         0.173    0.400
    depth / semantic   g_sem           0.319    0.249
    exact 0 and 1      g_depth         0.725    0.565   per element, in units of 4 * 2^-24 relative
    exact 0 and 1      g_sem           0.573    0.483   per element
    render, textured   loss_color      0.015    0.012
    render, textured   loss_ssim       1.956    0.779
    render, textured   loss_depth      0.011    0.010
    render, textured   g_render*       7.423    3.330   size_65x127 5.871 / 3.096, size_4161x5 2.447 / 1.409
    render, textured   g_depth*        0.086    0.086
    smooth_17x65       loss_ssim     300.357   19.248
    smooth_17x65       g_render0     479.917  747.899   1.56 x e_torch
    smooth_17x65       g_render1     644.693  768.353   1.19 x e_torch
    smooth_17x65       g_render2     717.879  664.008   0.92 x e_torch
    ssim(), C = 1      value           0.013    0.000
    ssim(), C = 1      g_img2          3.255    1.451

Every quantity whose oracle is exactly 0 came out exactly 0: the losses and gradients with no row in the label mask, the
gradients of the loss whose upstream gradient is 0, colour and SSIM with everything masked, the render gradients outside
the mask, the depth gradients on an exact tie.  The smooth pair stays within the factor 2 that every other case has
(1.56 at worst), so no case carries a factor of its own.  The depth labels are bit for bit in all 20 (ds, D) cases.
"""
import pytest
import torch

from ocrfdet_amd import losses
from tests import losses_oracle as lo

pytestmark = pytest.mark.gpu


def test_the_kernel_constants_the_shapes_rest_on():
    lo.assert_kernel_constants()


@pytest.mark.parametrize('D', lo.LABEL_D)
@pytest.mark.parametrize('ds', lo.LABEL_DS)
def test_depth_labels_bit_for_bit(cuda, ds, D):
    c = lo.label_case(ds, D)
    got = losses.depth_labels(c.gt_depth.to(cuda), c.gt_semantic.to(cuda), c.cfg, D, ds)
    assert lo.same_labels(got, c.want)


@pytest.mark.parametrize('name', list(lo.DS_SPECS))
def test_depth_semantic_loss_against_float64(cuda, name):
    c = lo.ds_case(name)
    lo.check(c, lo.ds_fused(c, cuda))


@pytest.mark.parametrize('name', list(lo.RENDER_SPECS))
def test_render_losses_against_float64(cuda, name):
    c = lo.render_case(name)
    lo.check(c, lo.render_fused(c, cuda))


def test_ssim_on_one_channel_against_float64(cuda):
    """``losses.ssim``: K = 1, no mask, no depth term."""
    c = lo.ssim_case()
    lo.check(c, lo.ssim_run(losses.ssim, c, device=cuda))


def test_inputs_without_grad_get_none_and_leave_the_other_gradients_to_the_bit(cuda):
    """Production: ``render_depth_G`` (the second render depth) does not require grad; once one render does not
    either."""
    c = lo.render_case('batch3_17x65')
    full = lo.render_fused(c, cuda)
    names = ('g_render0', 'g_render1', 'g_render2', 'g_depth0', 'g_depth1', 'g_depth2')
    for off in (('g_depth1',), ('g_depth1', 'g_render2'), ('g_depth1', 'g_render0')):
        got = lo.render_fused(c, cuda, requires=tuple(n not in off for n in names))
        for n in names:
            if n in off:
                assert got[n] is None, n
            else:
                assert torch.equal(got[n].view(torch.int32), full[n].view(torch.int32)), (off, n)
        for n in ('loss_color', 'loss_ssim', 'loss_depth'):
            assert torch.equal(got[n], full[n])
