"""``GraphedNeck``: ``OcRFViewTransformerFull`` inference as one hipGraph launch per call."""
import random

import torch

from . import _lib, neck_ops
from .neck_geometry import CALIB, calib_on_device


class GraphedNeck:
    """``OcRFViewTransformerFull`` inference (pre-filter + ``view_transform``) as ONE hipGraph launch per call for fixed
    shapes — with a static calibration (``accelerate=True``: the geometry is cached outside the graph) or, with
    ``module.device_geometry`` and the calibration tensors on the GPU, with the per-forward geometry INSIDE the graph
    (``accelerate=False``, the reference's working mode: calibration algebra, both index preparations and everything after
    them replay as one launch; the calibration values are copied into the graph's static inputs on every call):

        neck = GraphedNeck(module, example_input, example_depthnet_out)   # captures
        bev_feat, depth, (bev_mask, semantic), extras = neck(input, depthnet_out)

    ``input`` is the 12-entry ``img_inputs`` list, ``depthnet_out`` what ``module.depth_net`` returns (B*N, D+2+C, H, W);
    their values are copied into the static buffers the graph reads (image features, raw images and the DepthNet output —
    the calibration is frozen with the geometry).  The only per-call host decision, the random camera of each sample
    (view_transformer_ocrf.py:1081), is staged through two small static device tensors.  The three independent strands of
    the step run as parallel branches of the graph (``_core_fused``).  Outputs are static tensors, overwritten by the next
    call.  Eval mode, forward only."""

    def __init__(self, module, example_input, example_depthnet_out, warmup=3, parallel_branches=True,
                 capture_stream=None):
        self.per_forward_geometry = not module.accelerate
        if self.per_forward_geometry and not (module.device_geometry is not False and calib_on_device(example_input)):
            raise RuntimeError('GraphedNeck needs accelerate=True (geometry cached across calls), or the calibration '
                               'tensors on the GPU with module.device_geometry not switched off (geometry inside '
                               'the graph): the host formulation of the calibration algebra cannot be captured')
        if module.training:
            raise RuntimeError('GraphedNeck is inference only: call module.eval() first')
        self.module = m = module
        dev = example_input[0].device
        self.device = dev
        self.inputs = [t.clone() if torch.is_tensor(t) else t for t in example_input]
        self.depthnet_out = example_depthnet_out.detach().float().contiguous().clone()
        self.batch = self.inputs[0].shape[0]
        with torch.no_grad():
            self._body(None)                       # geometry, packs, workspaces, MIOpen algorithms
            if self.per_forward_geometry:
                # only the camera choice is staged; the rows follow from the in-graph geometry
                self._cams = dict(cam_sel=torch.zeros(self.batch, dtype=torch.int32, device=dev), packed=None,
                                  cam_idx_list=[0] * self.batch)
            else:
                self._cams = m.stage_cameras(m._geo, [0] * self.batch, dev)
            m.parallel_branches = parallel_branches
            try:
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(warmup):
                        self._body(self._cams)
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                try:
                    self._graph = torch.cuda.CUDAGraph(keep_graph=True)      # the raw graph stays inspectable
                    inspect = True
                except TypeError:
                    self._graph, inspect = torch.cuda.CUDAGraph(), False
                with torch.cuda.graph(self._graph, stream=capture_stream):
                    self._static_out = self._body(self._cams)
                if inspect:
                    # ROCm 7.2: a graph with memset nodes faults on replay after any hipMemcpyAsync on the stream (and
                    # every replay() stages the camera choice with one): refuse it here, loudly, instead of there
                    self.census = _lib.graph_census(self._graph)
                    if self.census['memset']:
                        raise _lib.OcrfHipError(
                            f"the captured neck graph holds {self.census['memset']} memset node(s) (a torch.zeros / "
                            '.zero_() / hipMemsetAsync inside the captured region): replaying it would fault on ROCm 7.2; '
                            'zero-fill with a kernel (e.g. tensor.fill_(0) on a non-empty tensor) or outside the graph')
                    self._graph.instantiate()
                # the graph has the raw pointers of the library's scratch buffers baked in: keep those
                # buffers alive for the graph's lifetime, whatever later eager calls make of their tags
                self._scratch = _lib.workspace.hold(dev)
            finally:
                m.parallel_branches = False

    def _body(self, cameras):
        m = self.module
        depth, fdepth, sem, feat_cl = neck_ops.prefilter(self.depthnet_out, m.D, m.out_channels, m.depth_threshold,
                                                         m.semantic_threshold)
        bev, _, bev_mask, extras = m.view_transform(self.inputs, fdepth, None, feat_cl, cameras=cameras)
        return bev, depth, (bev_mask, sem), extras

    def replay(self, cam_idx_list=None):
        """Replay on the values already in the static buffers (``self.inputs``, ``self.depthnet_out``)."""
        if cam_idx_list is None:
            cam_idx_list = [random.randint(0, 5) for _ in range(self.batch)]
        if self.per_forward_geometry:
            self._cams['cam_sel'].copy_(self.module._small_h2d(torch.tensor(list(cam_idx_list), dtype=torch.int32),
                                                               self.device))
            self._cams['cam_idx_list'] = list(cam_idx_list)
        else:
            self.module.stage_cameras(self.module._geo, cam_idx_list, self.device, out=self._cams)
        self._graph.replay()
        bev, depth, masks, ex = self._static_out
        return bev, depth, masks, list(ex[:5]) + [list(cam_idx_list)] + list(ex[6:])

    def __call__(self, input, depthnet_out, cam_idx_list=None):
        # image features and the three raw-image variants; with the geometry inside the graph also the calibration
        for i in (0, 8, 9, 10) + (CALIB if self.per_forward_geometry else ()):
            if torch.is_tensor(input[i]) and input[i] is not self.inputs[i]:
                self.inputs[i].copy_(input[i], non_blocking=True)
        if depthnet_out is not self.depthnet_out:
            self.depthnet_out.copy_(depthnet_out, non_blocking=True)
        return self.replay(cam_idx_list)
