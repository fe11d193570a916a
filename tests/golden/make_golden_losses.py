"""Generates ``tests/golden/losses.npz``: the reference's own training losses of the neck, run on the CPU.

    python tests/golden/make_golden_losses.py

Imports the reference's ``view_transformer_ocrf`` behind the stubs of ``_ref_import.py`` (read-only tree, nothing
copied) and calls, on a small seeded batch (B = 2, 6 cameras 32 x 176, downsample 16, depth bins [1, 60, 0.5]):

* ``OcRFViewTransformerFull.get_loss`` (:1354-1417) twice, with the module-global ``iteration`` set on either side of
  3862 * 2 (box mask off / on), through ``get_downsampled_gt_depth_and_semantic`` (:1203-1282),
  ``get_depth_and_semantic_loss`` (:1284-1314), ``Box2dtoMask`` (:1337-1352) and MVSGaussian's SSIM;
* ``ProbNet.get_bev_mask_loss`` / ``get_bev_opacity_loss`` (:177-201).

``get_loss`` is called unbound on a shim that carries the attributes it reads.  ``visualize_images`` (undefined in the
reference) is stubbed and ``gt_images`` gets B + 1 rows: the extra row only feeds that debug line (:1373).  Stored:
the inputs, the labels, the 5 losses, the box masks, the ProbNet dicts and the autograd gradients of the loss sums.

Size: the images and render depths lie on a k / 256 grid and are stored as the uint8 k (``decode`` restores the
float32 values exactly), the logits on a k / 16 grid as int8 k.  The depth / semantic gradients do not depend on the box
mask and are stored once (``grad_depth``, ``grad_semantic``); with the mask off the render gradient is stored for the
first render only (the other two go through the same code path and are stored with the mask on).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

B, N, H, W, DS = 2, 6, 32, 176, 16
DEPTH = [1.0, 60.0, 0.5]
D = int(round((DEPTH[1] - DEPTH[0]) / DEPTH[2]))
CAMS = [1, 4]
BEV = 16


def make_inputs(seed=0):
    rng = np.random.default_rng(seed)
    gd = np.zeros((B, N, H, W), np.float32)
    hit = rng.random((B, N, H, W)) < 0.08
    gd[hit] = rng.uniform(0.2, 70.0, hit.sum()).astype(np.float32)           # below d0 and above d1 as well
    sem_patch = np.repeat(np.repeat(rng.random((B, N, H // DS, W // DS)) < 0.4, DS, 2), DS, 3)
    gs = ((rng.random((B, N, H, W)) < 0.5) & hit & sem_patch).astype(np.float32)
    # exactly d1 (kept: the range test is strict, but its bin D + 1 is out)
    gd[0, 0, 5, 7] = 60.0
    gs[0, 0, 5, 7] = 1.0
    # patch (0, 0, row 1, col 2): its only semantic pixels sit at d1 -> a NaN soft row
    gd[0, 0, 16:32, 32:48] = 0.0
    gs[0, 0, 16:32, 32:48] = 0.0
    gd[0, 0, 20, 40], gs[0, 0, 20, 40] = 60.0, 1.0
    gd[0, 0, 25, 33], gs[0, 0, 25, 33] = 60.0, 1.0
    gd[0, 0, 30, 45], gs[0, 0, 30, 45] = 30.0, 0.0
    # empty patches; a patch whose only semantic pixel is below d0
    gd[1, 3, 0:16, 0:16] = 0.0
    gs[1, 3, 0:16, 0:16] = 0.0
    gd[1, 2, 16:32, 160:176] = 0.0
    gs[1, 2, 16:32, 160:176] = 0.0
    gd[1, 2, 20, 170], gs[1, 2, 20, 170] = 0.5, 1.0
    h, w = H // DS, W // DS
    # logits on a 1/16 grid (int8), images and render depths on a 1/256 grid (uint8): see the module docstring
    depth_logits = np.clip(np.round(rng.standard_normal((B * N, D, h, w)) * 32), -127, 127).astype(np.int8)
    sem_logits = np.clip(np.round(rng.standard_normal((B * N, 2, h, w)) * 16), -127, 127).astype(np.int8)
    q = lambda a: np.clip(np.round(a * 256), 0, 255).astype(np.uint8)      # noqa: E731
    gt_images = q(rng.uniform(0, 1, (B + 1, 3, H, W)))
    gt_images[B] = 0                                  # the extra row only feeds the dropped debug line
    renders = [q(np.clip(gt_images[:B] / 256.0 + rng.normal(0, s, (B, 3, H, W)), 0, 1)) for s in (0.05, 0.1, 0.2)]
    rdepths = [q(rng.uniform(0, 1, (B, 1, H, W))) for _ in range(3)]
    # boxes in the 1600-wide original frame; at W = 176 the scale is 0.11 and y is shifted by -158
    boxes0 = np.array([[100, 1450, 600, 1800],        # y2 past H
                       [1200, 1450, 2000, 1600],      # x2 past W
                       [700, 500, 900, 1600],         # y1 negative (-103 -> -71 -> 0)
                       [300, 1255, 800, 1528],        # y1 = -20 -> 12, y2 = 10: empty
                       [50, 1255, 200, 1300],         # y1 = -20 -> 12, y2 = -15 -> 17
                       [-200, 1500, 100, 1600]],      # x1 = -22 -> 154, x2 = 11: empty
                      np.float32)
    boxes = np.zeros((B, N, 6, 4), np.float32)
    counts = np.zeros((B, N), np.int32)
    for b in range(B):
        for n in range(N):
            k = int(rng.integers(1, 4))
            boxes[b, n, :k] = boxes0[rng.permutation(6)[:k]]
            counts[b, n] = k
    boxes[0, CAMS[0]] = boxes0
    counts[0, CAMS[0]] = 6
    counts[1, CAMS[1]] = 0                            # a sample with no boxes
    gt_bev = (rng.random((B, BEV, BEV)) < 0.3).astype(np.float32)
    bev_logits = rng.standard_normal((B, 1, BEV, BEV)).astype(np.float32)
    opa_logits = rng.standard_normal((B, 1, BEV, BEV)).astype(np.float32)
    return dict(gt_depth=gd, gt_semantic=gs, depth_logits=depth_logits, sem_logits=sem_logits, gt_images=gt_images,
                render=renders[0], render_G=renders[1], render_N=renders[2], render_depth=rdepths[0],
                render_depth_G=rdepths[1], render_depth_N=rdepths[2], boxes=boxes, box_counts=counts,
                cams=np.array(CAMS, np.int32), gt_bev=gt_bev, bev_logits=bev_logits, opa_logits=opa_logits)


def decode(arrays):
    """The float32 tensors of a fixture dict: uint8 k -> k / 256, int8 k -> k / 16 (both exact)."""
    out = {}
    for k, v in arrays.items():
        v = np.asarray(v)
        if v.dtype == np.uint8:
            v = v.astype(np.float32) / np.float32(256)
        elif v.dtype == np.int8:
            v = v.astype(np.float32) / np.float32(16)
        out[k] = torch.from_numpy(np.ascontiguousarray(v))
    return out


def box_lists(inp):
    return [[torch.from_numpy(inp['boxes'][b, n, :inp['box_counts'][b, n]]) for n in range(N)] for b in range(B)]


def main():
    import _ref_import
    _, vto, _, _ = _ref_import.install()
    inp = make_inputs()
    t = decode(inp)
    shim = types.SimpleNamespace(grid_config=dict(depth=DEPTH), downsample=DS, D=D, loss_depth_weight=3.0,
                                 loss_semantic_weight=25, color_crit=torch.nn.MSELoss(reduction='mean'))
    cls = vto.OcRFViewTransformerFull
    for name in ('get_downsampled_gt_depth_and_semantic', 'get_depth_and_semantic_loss', 'depth_l1_loss', 'Box2dtoMask',
                 'get_loss'):
        setattr(shim, name, types.MethodType(getattr(cls, name), shim))
    shim.visualize_images = lambda *a, **k: None
    out = dict(inp)
    out['D'] = np.int32(D)
    out['ds'] = np.int32(DS)
    out['depth_cfg'] = np.array(DEPTH, np.float64)
    dl, sl = shim.get_downsampled_gt_depth_and_semantic(t['gt_depth'].clone(), t['gt_semantic'].clone())
    out['depth_labels'], out['semantic_labels'] = dl.numpy(), sl.numpy()
    H_, W_ = inp['gt_images'].shape[2:]
    for b in range(B):
        bx = box_lists(inp)[b][CAMS[b]]
        out[f'box_mask_{b}'] = shim.Box2dtoMask(bx, W_, H_).numpy()
    for tag, it in (('nomask', 3862 * 2 - 1), ('mask', 3862 * 2)):
        vto.iteration = it
        depth = t['depth_logits'].softmax(1).requires_grad_(True)
        sem = t['sem_logits'].softmax(1).requires_grad_(True)
        rs = [t[k].clone().requires_grad_(True) for k in ('render', 'render_G', 'render_N')]
        rd, rdG, rdN = t['render_depth'].clone().requires_grad_(True), t['render_depth_G'], \
            t['render_depth_N'].clone().requires_grad_(True)
        ls = shim.get_loss(depth, sem, t['gt_depth'].clone(), t['gt_semantic'].clone(), box_lists(inp), CAMS,
                           rs[0], t['gt_images'], rs[1], rs[2], rd, rdG, rdN)
        assert vto.iteration == it + 1
        out[f'losses_{tag}'] = np.array([float(v) for v in ls], np.float64)
        sum(ls).backward()
        for name, v in (('depth', depth), ('semantic', sem)):
            if f'grad_{name}' in out:
                assert np.array_equal(out[f'grad_{name}'], v.grad.numpy()), 'the label losses do not see the box mask'
            out[f'grad_{name}'] = v.grad.numpy()
        named = [('render', rs[0]), ('render_depth', rd), ('render_depth_N', rdN)]
        if tag == 'mask':
            named += [('render_G', rs[1]), ('render_N', rs[2])]
        for name, v in named:
            out[f'grad_{tag}_{name}'] = v.grad.numpy()
    torch.manual_seed(0)
    prob = vto.ProbNet(in_channels=16, with_centerness=True, bev_size=(BEV, BEV))
    bev = t['bev_logits'].clone().requires_grad_(True)
    opa = t['opa_logits'].clone().requires_grad_(True)
    m = prob.get_bev_mask_loss(t['gt_bev'], bev)
    o = prob.get_bev_opacity_loss(t['gt_bev'], opa.squeeze(1))
    for k, v in list(m.items()) + list(o.items()):
        out[f'prob_{k}'] = np.float64(float(v))
    (sum(m.values()) + sum(o.values())).backward()
    out['grad_bev_logits'], out['grad_opa_logits'] = bev.grad.numpy(), opa.grad.numpy()
    path = os.path.join(HERE, 'losses.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB)')
    for tag in ('nomask', 'mask'):
        print(tag, out[f'losses_{tag}'])
    print('NaN label rows:', int(np.isnan(out['depth_labels']).any(1).sum()), 'soft rows:',
          int((out['semantic_labels'][:, 1] > 0).sum()))


if __name__ == '__main__':
    main()
