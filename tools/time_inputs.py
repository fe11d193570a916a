"""Timing of the input stage (``ocrfdet_amd.inputs``) at the reference shape: frames of 900 x 1600 to 256 x 704 with
training-mode augmentations (configs/ocrfdet/ocrfdet.py: resize -0.06 ... 0.11, rotate +-5.4, flip), 6 cameras x 3 frames
per sample: 18 frames (one sample) and 144 frames (``samples_per_gpu = 8``).

* fused: ``prepare_images(..., fused=True)``, three launches of ``ocrf_image_prep`` and one upload of the tables.  Device
  time and launch count from the torch profiler; wall time per call from a host clock around synchronised blocks, once
  with the same augmentations every call (the pinned table is cached: what testing sees) and once with fresh draws every
  call and the caches emptied (coefficients and tables rebuilt on the host: the most training can cost); synchronising
  torch calls counted with ``torch.cuda.set_sync_debug_mode('warn')``; the kernels' algorithmic bytes against the
  MI355X's measured HBM copy rate.
* the reference's formulation on the host, restated here with Pillow and numpy in one process
  (mmdet3d/datasets/pipelines/loading.py:1071-1123: two ``resize`` + ``crop`` per frame, flip, rotate, two
  normalisations and the float copy), decoded frames in memory: no JPEG decoding on either side.
* ``prepare_images_torch``, the numpy form the CPU and ``fused=False`` take (18 frames only: it is slow).
* the point labels: ``point_label_maps`` for the sample's cameras with 30 000 points each, fused against the numpy form.

No ratio is required: the acceptance conditions are bit equality (checked here once per case against Pillow) and the
launch structure.

    python tools/time_inputs.py [--iters N] [--out profiles/inputs_time.txt]

Every case runs in a child process of its own under a time limit (``--limit`` seconds); the first case that fails or runs
out of time ends the run.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [18, 144]
N_CAMS, N_FRAMES = 6, 3
SRC, INPUT_SIZE = (900, 1600), (256, 704)
DATA_CONFIG = dict(input_size=INPUT_SIZE, src_size=SRC, resize=(-0.06, 0.11), rot=(-5.4, 5.4), flip=True,
                   crop_h=(0.0, 0.0), resize_test=0.0)
HBM_TBS = 6.29                               # MI355X_MICROARCH: measured float4 copy rate


def draw_augs(cameras, rng):
    from ocrfdet_amd import inputs
    return [inputs.sample_augmentation(DATA_CONFIG, *SRC, True, rng) for _ in range(cameras)]


def reference_host(frames, augs, mean, stdinv):
    """loading.py:1071-1123 for every frame, Pillow + numpy: returns the three float arrays."""
    import numpy as np
    from PIL import Image
    F = len(frames) // len(augs)
    outs = ([], [], [])
    norm = lambda a: ((a[:, :, ::-1].astype(np.float32) - mean) * stdinv).transpose(2, 0, 1)      # noqa: E731
    for m, frame in enumerate(frames):
        _, dims, crop, flip, rotate = augs[m // F]
        img = Image.fromarray(frame)
        wo_aug = img.resize(dims).crop(crop)
        aug = img.resize(dims).crop(crop)
        if flip:
            aug = aug.transpose(method=Image.FLIP_LEFT_RIGHT)
        aug = aug.rotate(rotate)
        outs[0].append(norm(np.array(aug)))
        outs[1].append(norm(np.array(wo_aug)))
        if flip:
            wo_aug = wo_aug.transpose(method=Image.FLIP_LEFT_RIGHT)
        outs[2].append(np.ascontiguousarray(np.array(wo_aug).astype(np.float32).transpose(2, 0, 1)))
    return tuple(np.stack(o) for o in outs)


def algorithmic_bytes(augs, M):
    """Bytes the three kernels have to move: the source rows the crop needs, the uint8 intermediate and the cropped image
    written and read once each, and the nine float planes."""
    from ocrfdet_amd import inputs
    fH, fW = INPUT_SIZE
    F = M // len(augs)
    checked = tuple(inputs._aug4(a) for a in augs)
    table, _ = inputs._image_table(checked, *SRC, fH, fW)
    total = 0
    for g in range(len(augs)):
        rows = int(table[g * 16 + 1])
        total += F * (rows * SRC[1] * 3 + 2 * rows * fW * 3 + 2 * fH * fW * 3 + 9 * fH * fW * 4)
    return total + table.nbytes


def _kernel_times(fn, reps=5):
    """{short kernel name: device us per call} from the torch profiler."""
    import collections
    import re

    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    times = collections.OrderedDict()
    for e in p.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and e.name:
            m = re.search(r'(\w+_kernel)', e.name)
            name = m.group(1) if m else e.name
            times[name] = times.get(name, 0.0) + (e.device_time_total if hasattr(e, 'device_time_total')
                                                  else e.cuda_time_total) / reps
    return times


def run_case(M, iters):
    import numpy as np
    import torch
    from time_bev_encoder import _wall
    from time_detector import _profile, _syncs
    from ocrfdet_amd import inputs
    dev = torch.device('cuda:0')
    cameras = M // N_FRAMES
    rng = np.random.RandomState(0)
    base = rng.randint(0, 256, (N_FRAMES * 2, *SRC, 3)).astype(np.uint8)
    frames = np.stack([base[m % len(base)] for m in range(M)])          # M frames from 6 distinct images
    augs = draw_augs(cameras, rng)
    mean, stdinv = inputs._norm_constants(inputs.MEAN, inputs.STD)
    d_frames = torch.from_numpy(frames).to(dev)

    fused = lambda: inputs.prepare_images(d_frames, augs, INPUT_SIZE)      # noqa: E731
    for _ in range(3):
        got = fused()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = reference_host(frames, augs, mean, stdinv)
    ref_s = time.perf_counter() - t0
    same = [bool(np.array_equal(g.cpu().numpy(), w)) for g, w in zip(got, want)]
    print(f'{M} frames of {SRC[0]} x {SRC[1]} -> {INPUT_SIZE[0]} x {INPUT_SIZE[1]}, {cameras} cameras x {N_FRAMES} frames, '
          f'training augmentations: fused against Pillow + numpy bit-equal (imgs, imgs_wo_aug, imgs_wo_norm): {same}')
    assert all(same)
    del got, want

    fresh_sets = [draw_augs(cameras, rng) for _ in range(8)]
    state = dict(i=0)

    def fresh():
        state['i'] += 1
        return inputs.prepare_images(d_frames, fresh_sets[state['i'] % len(fresh_sets)], INPUT_SIZE)
    n = max(iters // (1 if M <= 18 else 4), 2)
    (fb, fm), = _wall([fused], n)

    def fresh_cold():                                    # nothing cached: every call builds its coefficients and its table
        inputs.resample_table.cache_clear()
        inputs._image_table.cache_clear()
        inputs._pinned_image_table.cache_clear()
        return fresh()
    (cb, cm), = _wall([fresh_cold], n)
    launches, dev_ms, _ = _profile(fused)
    nbytes = algorithmic_bytes(augs, M)
    print(f'  fused (ocrf_image_prep): {dev_ms:.3f} ms device ({dev_ms / M * 1e3:.1f} us per frame), {launches:.0f} launches '
          f'(3 kernels + the table upload), wall best {fb:.3f} / median {fm:.3f} ms with the table cached, best {cb:.3f} / '
          f'median {cm:.3f} ms with fresh draws and every table rebuilt, {_syncs(fused)} synchronisations')
    print('    per call: ' + ', '.join(f'{k} {v:.1f} us' for k, v in _kernel_times(fused).items()))
    print(f'    {nbytes / 1e6:.0f} MB algorithmic -> {nbytes / dev_ms / 1e9:.2f} TB/s, {nbytes / dev_ms / 1e9 / HBM_TBS:.0%} of '
          f'the {HBM_TBS} TB/s copy rate')
    t0 = time.perf_counter()
    reference_host(frames, augs, mean, stdinv)
    ref_s = min(ref_s, time.perf_counter() - t0)
    print(f'  reference formulation on the host (Pillow + numpy, one process): {ref_s * 1e3:.0f} ms '
          f'({ref_s / M * 1e3:.1f} ms per frame), best of 2')
    if M <= 18:
        host_frames = torch.from_numpy(frames)
        t0 = time.perf_counter()
        inputs.prepare_images_torch(host_frames, augs, INPUT_SIZE)
        print(f'  prepare_images_torch (numpy, CPU tensors): {(time.perf_counter() - t0) * 1e3:.0f} ms, one run')

    # point labels of the same cameras
    P = 30000
    pts = np.concatenate([rng.uniform(0, SRC[1], (cameras, P, 1)), rng.uniform(0, SRC[0], (cameras, P, 1)),
                          rng.uniform(1, 60, (cameras, P, 1)), rng.choice([-1.0, 0.0, 3.0], (cameras, P, 1))], 2)
    d_pts = torch.from_numpy(pts).to(dev)
    counts = torch.full((cameras,), P, dtype=torch.int32)
    d_counts = counts.to(dev)
    labels = lambda: inputs.point_label_maps(d_pts, d_counts, augs, INPUT_SIZE)      # noqa: E731
    for _ in range(3):
        got = labels()
    t0 = time.perf_counter()
    want = inputs.point_label_maps_torch(torch.from_numpy(pts), counts, augs, INPUT_SIZE)
    host_s = time.perf_counter() - t0
    same = [bool(torch.equal(g.cpu(), w)) for g, w in zip(got, want)]
    assert all(same)
    (lb, lm), = _wall([labels], n * 4)
    launches, dev_ms, _ = _profile(labels)
    print(f'  point labels, {cameras} cameras x {P} points: fused (ocrf_point_labels) {dev_ms * 1e3:.1f} us device, '
          f'{launches:.0f} launches (2 kernels + the parameter upload), wall best {lb * 1e3:.1f} / median {lm * 1e3:.1f} us, '
          f'{_syncs(labels)} synchronisations; point_label_maps_torch (numpy) {host_s * 1e3:.0f} ms; bit-equal: {same}')
    print('    per call: ' + ', '.join(f'{k} {v:.1f} us' for k, v in _kernel_times(labels).items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--limit', type=int, default=240, help='seconds per case')
    ap.add_argument('--case', type=int, default=None, help='(internal) run this one case in this process')
    a = ap.parse_args()
    if a.case is not None:
        import torch
        assert torch.cuda.is_available(), 'timing needs the GPU: there is no CPU fallback for a measurement'
        run_case(CASES[a.case], a.iters)
        return 0
    lines = []
    for k in range(len(CASES)):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--iters', str(a.iters)],
                               stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} ran out of its {a.limit} s: stopping', file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            print(f'case {CASES[k]} ended with status {p.returncode}: stopping', file=sys.stderr)
            return p.returncode or 1
        lines.append(p.stdout)
    if a.out:
        import PIL
        import torch
        with open(a.out, 'w') as f:
            f.write(f'torch {torch.__version__}, Pillow {PIL.__version__}; device time and launches from the torch profiler; '
                    'wall: host clock around synchronised blocks; synchronisations: warnings of '
                    'torch.cuda.set_sync_debug_mode\n' + ''.join(lines))
    return 0


if __name__ == '__main__':
    sys.exit(main())
