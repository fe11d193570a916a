"""Diagnostic: what the depth / final_T gradients cost in the rasteriser's backward, and whether adding them moved the
colour-only backward.  Shape: the neck's training render of a bench configuration (default cfg2) — every voxel's
Gaussian, ONE camera, as ``view_transform_core`` renders it per sample (``tools/time_neck_train.py`` drives it).

Three arms, alternated block by block, device time from the torch profiler (kernels only), median over the blocks:
  colour        ocrf_rasterize_backward of this tree's library
  parent        the same entry of another build of the library (``--parent-so``), e.g. the parent commit's:
                    python tools/time_raster_depth_grad.py --build-parent DIR [--rev HEAD~1]     (needs git, no GPU)
                    python tools/time_raster_depth_grad.py --parent-so DIR/ocrfdet_amd/csrc/libocrf_hip.so
  depth+final_T ocrf_rasterize_backward_depth with both gradients

All three are called straight through ctypes on the same buffers; the parent's library is a second CDLL in the process.
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parent(dest, rev):
    """Check ``rev``'s library sources out of git into ``dest`` and build them there (hipcc cross-compiles)."""
    os.makedirs(dest, exist_ok=True)
    tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, 'ocrfdet_amd/csrc', 'include'], check=True, stdout=subprocess.PIPE)
    subprocess.run(['tar', '-x', '-C', dest], input=tar.stdout, check=True)
    subprocess.check_call(['make', '-C', os.path.join(dest, 'ocrfdet_amd', 'csrc'), '-j8', 'libocrf_hip.so'],
                          stdout=subprocess.DEVNULL)
    print(os.path.join(dest, 'ocrfdet_amd', 'csrc', 'libocrf_hip.so'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('config', nargs='?', default='cfg2_6cam_2frame_bev200x200_render_hoa')
    ap.add_argument('--build-parent', metavar='DIR')
    ap.add_argument('--rev', default='HEAD~1')
    ap.add_argument('--parent-so')
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    a = ap.parse_args()
    if a.build_parent:
        return build_parent(a.build_parent, a.rev)

    import torch
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    from ocrfdet_amd import _lib, hotpath, synthetic
    from ocrfdet_amd import diff_gaussian_rasterization as dgr

    cfg = synthetic.CONFIGS[a.config]
    dev = torch.device('cuda:0')
    hp = hotpath.HotPath(cfg, dev)
    rc, g = hp.render_cams, hp.gauss
    H, W = cfg.input_size
    xyz = hp.voxel_xyz[0].reshape(-1, 3).contiguous()
    P = xyz.shape[0]
    cams = dgr.pack_cameras(rc['vm'][:1], rc['pm'][:1], rc['tfx'][:1], rc['tfy'][:1], H, W, dev)
    args = [t.detach().contiguous().float() for t in (xyz, g['rgb'], g['opacity'].reshape(-1), g['scales'], g['rotations'])]
    fwd = dgr.rasterize_views(*args, None, None, None, None, H, W, hp.bg, depth_mode='mean', packed_cameras=cams)
    gen = torch.Generator(dev).manual_seed(0)
    gcol = torch.randn(1, 3, H, W, device=dev, generator=gen)
    gdep, gfin = torch.randn(1, H, W, device=dev, generator=gen), torch.randn(1, H, W, device=dev, generator=gen)
    out = [torch.empty(P, k, device=dev) for k in (3, 3, 1, 3, 4)]
    fc, fd, ft, fn = fwd['color'], fwd['depth'].reshape(1, H, W).contiguous(), fwd['final_T'], fwd['n_contrib']
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    here = _lib.lib()
    protos = _lib.prototypes()

    def colour_arm(L):
        fn_ = L.ocrf_rasterize_backward
        fn_.restype, fn_.argtypes = protos['ocrf_rasterize_backward']
        ws = torch.empty(L.ocrf_rasterize_backward_workspace_bytes(P, 1), dtype=torch.uint8, device=dev)

        def run():
            err = fn_(P, 1, H, W, *map(ptr, args[:4]), 1.0, ptr(args[4]), ptr(cams), ptr(hp.bg), ptr(fc), ptr(ft), ptr(fn),
                      ptr(gcol), *map(ptr, out), None, ptr(ws), ws.numel(), _lib.stream_ptr(dev))
            assert err == 0, err
        return run

    ws10 = torch.empty(here.ocrf_rasterize_backward_depth_workspace_bytes(P, 1), dtype=torch.uint8, device=dev)

    def depth_arm():
        err = here.ocrf_rasterize_backward_depth(
            P, 1, H, W, *map(ptr, args[:4]), 1.0, ptr(args[4]), None, ptr(cams), ptr(hp.bg), ptr(fc), ptr(fd), ptr(ft),
            ptr(fn), ptr(gcol), ptr(gdep), ptr(gfin), *map(ptr, out), None, None, ptr(ws10), ws10.numel(),
            _lib.stream_ptr(dev))
        assert err == 0, err

    arms = {'colour': colour_arm(here)}
    if a.parent_so:
        arms['parent'] = colour_arm(ctypes.CDLL(os.path.abspath(a.parent_so)))
    arms['depth+final_T'] = depth_arm

    def device_us(fn_):
        """-> (device time of all kernels, of the blend alone, of the preprocess backward alone) per call, in us."""
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
            for _ in range(a.iters):
                fn_()
            torch.cuda.synchronize()
        kern = [e for e in p.key_averages() if e.device_type == DeviceType.CUDA]
        part = lambda s: sum(e.self_device_time_total for e in kern if s in e.key) / a.iters      # noqa: E731
        return part(''), part('raster_blend_kernel'), part('raster_preprocess_backward')

    for fn_ in arms.values():
        for _ in range(3):
            fn_()
    torch.cuda.synchronize()
    rows = {k: [] for k in arms}
    for _ in range(a.blocks):
        for k, fn_ in arms.items():
            rows[k].append(device_us(fn_))
    print(f'{cfg.name}: P = {P}, one view {H} x {W}; device time per backward in us, median of {a.blocks} alternated blocks '
          f'of {a.iters} (min .. max of the blocks)')
    med = {}
    for k, r in rows.items():
        tot = [x[0] for x in r]
        med[k] = statistics.median(tot)
        print(f'  {k:14s} all kernels {med[k]:8.1f} ({min(tot):.1f} .. {max(tot):.1f})   blend {statistics.median(x[1] for x in r):8.1f}'
              f'   preprocess backward {statistics.median(x[2] for x in r):6.1f}')
    if 'parent' in med:
        tot = [x[0] for x in rows['parent']]
        print(f'  colour - parent: {med["colour"] - med["parent"]:+.1f} us; spread between the parent arm\'s blocks: '
              f'{max(tot) - min(tot):.1f} us')
    print(f'  depth+final_T / colour: {med["depth+final_T"] / med["colour"]:.3f}')


if __name__ == '__main__':
    main()
