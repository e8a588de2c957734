"""CenterNet after the network's last convolution, on the kernels of csrc/centernet.hip -- the reference's names and signatures
(models/det/centernet.py): ground truth (`centernet_ground_truth`, CenterNetGT), `modified_focal_loss`, `reg_l1_loss`, `gather_feature`
and `CenterNetDecoder`, and the detector itself: `CenterNet` = the ResNet trunk ending at res5 (FPNDetector with HAS_FPN = False: the
same stem, block loops, norms and plan, no pyramid) -> layers.CenternetDeconv -> layers.CenterHead, three losses and the decoder.

The seams of the detector are pixel-major bf16 with no NCHW / fp32 round trip: res5's stored block output is what the neck's forward_pm
reads, the neck's output what the head reads, the head's raw logits_pm / wr_pm what the loss and decode kernels read.  Backward: the
neck's d_x through ops.relu_bwd_bf16 against res5's output is res5's g_out in the trunk's convention (dL/d(pre-activation), masked), then
the trunk's own backward loop.  The neck's and head's fp32 masters, gradients and norm statistics live in the model's parameter arena
and LiveNorms (the layers' adopt()), so the fused optimizer launch, ModelEMA, GradClip, GradBuckets, broadcast_parameters and checkpoints
see them; their activations and workspaces stay layer-owned, and their weight gradients run on the main stream.
Inference decodes the raw head outputs (K = 100, reg given) and maps the boxes to the image for the whole batch in one launch
(bd_centernet_boxes_to_image) from six host-built floats per image.  Not built: fp8 weights.  The pipeline of AUG.TRAIN_VALUE (CenterAffine and the
colour augmentations) reaches pre_process as a data/raw.py CenterNetRawCollator batch and runs in bd_affine_jitter_normalize.

Tensors are the reference's: NCHW fp32 on the HIP device (host tensors raise: there is no CPU path).  The kernels read the head's
convolution output -- pixel-major bf16 LOGITS -- so the functions that take probabilities, as the reference's do, turn them back into
logits and round them to bf16 on the way in; a model step hands the convolution output to basedet_amd.ops directly.

What runs where: `centernet_ground_truth`, the two losses (value and gradient, through a torch.autograd.Function) and
`CenterNetDecoder.decode` are one HIP entry each.  `gather_feature`, `pseudo_nms` and `topk_score` are the reference's stand-alone
helpers, kept as device tensor indexing / pooling for callers that use them on their own (decode does not: its kernel fuses them).
CenterNetGT's per-image methods and `transform_boxes` / `generate_src_and_dst` are host numpy, as gaussian2D and transform_boxes
are in the reference."""
import numpy as np
import torch
import torch.nn.functional as TF

from basedet_amd import ops
from basedet_amd.layers._pm import need_device_all, round_up8, round_up32
from basedet_amd.utils.registry import registers

from . import params as P
from .adopted import AdoptedParts
from .fpn_base import FPNDetector

__all__ = ["CenterNet", "CenterNetGT", "CenterNetDecoder", "centernet_ground_truth", "gather_feature", "modified_focal_loss", "reg_l1_loss"]

_MODULE = "basedet_amd.models.centernet"          # (named in the refusal of a host tensor)


def _to_pm(x, ld):
    """(N, C, H, W) fp32 -> pixel-major bf16 (N*H*W, ld), the slots >= C zero."""
    n, c, h, w = x.shape
    out = torch.zeros((n * h * w, ld), dtype=torch.bfloat16, device=x.device)
    out[:, :c] = x.permute(0, 2, 3, 1).reshape(n * h * w, c)
    return out


def _from_pm(t, n, c, h, w):
    return t[:, :c].float().reshape(n, h, w, c).permute(0, 3, 1, 2)


def centernet_ground_truth(gt_boxes, num_gt, cfg):
    """CenterNet.get_ground_truth (centernet.py:74-127): gt_boxes fp32 (N, G, 5) xyxy + 1-based label, num_gt int32 (N,) -- the img_info
    count of the reference -- and the config -> gt_dict {score_map (N, K, H, W), wh, reg (N, T, 2), reg_mask (N, T), index int32 (N, T)}
    plus num_pos (1,), the number of map elements equal to 1.  score_map is a view of the kernel's pixel-major (N, H*W, K) map."""
    need_device_all((gt_boxes, num_gt), _MODULE)
    m = cfg.MODEL
    K, T = int(cfg.DATA.NUM_CLASSES), int(m.HEAD.TENSOR_DIM)
    H, W = (int(v) for v in m.OUTPUT_SIZE)
    out = ops.centernet_targets(gt_boxes.float().contiguous(), num_gt.to(torch.int32).contiguous(), K, H, W, T, 1 / m.HEAD.DOWN_SCALE,
                                m.HEAD.MIN_OVERLAP)
    out["score_map"] = out["score_map"].view(gt_boxes.shape[0], H, W, K).permute(0, 3, 1, 2)
    return out


def gather_feature(fmap, index, mask=None, use_transform=False):
    """centernet.py:189-205: rows `index` (B, T) of fmap (B, P, C) -- or of an NCHW map with use_transform -- optionally only the rows
    where mask is set, flattened to (-1, C)."""
    need_device_all((fmap, index, mask), _MODULE)
    if use_transform:
        fmap = fmap.flatten(2).transpose(1, 2)
    C = fmap.shape[-1]
    rows = torch.gather(fmap, 1, index.long().unsqueeze(-1).expand(-1, -1, C))
    if mask is None:
        return rows
    return rows[mask.bool()].reshape(-1, C)


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        n, k, h, w = pred.shape
        ld = round_up8(k)
        p = pred.float()
        logits = _to_pm(torch.log(p) - torch.log1p(-p), ld)
        gmap = gt.float().permute(0, 2, 3, 1).reshape(n * h * w, k).contiguous()
        num_pos = (gmap == 1).sum().float().reshape(1)
        loss = torch.zeros(1, dtype=torch.float32, device=pred.device)
        d = torch.empty_like(logits)
        ops.centernet_focal_fwd_bwd(logits, gmap, n * h * w, k, ld, num_pos, 1.0, 1.0, loss, d)
        den = p * (1 - p)                       # d logit / d p = 1 / (p (1 - p)); the kernel's gradient is 0 where p is 0 or 1 (clipped)
        g = _from_pm(d, n, k, h, w)
        ctx.save_for_backward(torch.where(den > 0, g / den, torch.zeros_like(g)))
        ctx.dtype = pred.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return (g * gout).to(ctx.dtype), None


def modified_focal_loss(pred, gt):
    """centernet.py:218-242: pred the head's probabilities (N, K, H, W), gt the score map."""
    if pred.shape != gt.shape or pred.dim() != 4:
        raise ValueError("modified_focal_loss: pred and gt are (N, K, H, W) tensors of one shape")
    need_device_all((pred, gt), _MODULE)
    return _Focal.apply(pred, gt)


class _RegL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, mask, index, target):
        n, c, h, w = output.shape
        t = index.shape[1]
        pm = _to_pm(output.float(), 8)
        loss = torch.zeros(1, dtype=torch.float32, device=output.device)
        d = torch.empty_like(pm)
        ops.centernet_l1_fwd_bwd(pm, 8, 0, index.to(torch.int32).contiguous(), mask.float().contiguous(), target.float().contiguous(),
                                 n, h, w, t, 1.0, 1.0, loss, d)
        ctx.save_for_backward(_from_pm(d, n, c, h, w))
        ctx.dtype = output.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return (g * gout).to(ctx.dtype), None, None, None


def reg_l1_loss(output, mask, index, target):
    """centernet.py:208-215: output (N, 2, H, W), mask (N, T), index (N, T), target (N, T, 2)."""
    if output.shape[1] != 2 or tuple(target.shape) != tuple(index.shape) + (2,) or mask.shape != index.shape:
        raise ValueError("reg_l1_loss: output (N, 2, H, W), mask and index (N, T), target (N, T, 2)")
    need_device_all((output, mask, index, target), _MODULE)
    return _RegL1.apply(output, mask, index, target)


class CenterNetDecoder:

    @staticmethod
    def decode(fmap, wh, reg=None, cat_spec_wh=False, K=100):
        """centernet.py:247-291: fmap the head's probabilities (B, C, H, W), wh / reg (B, 2, H, W) -> (bboxes (B, K, 4), scores (B, K, 1),
        clses (B, K, 1) float32).  Ties come out by class, then pixel (bd_centernet_decode)."""
        if cat_spec_wh:
            raise ValueError("CenterNetDecoder.decode: cat_spec_wh=True (a wh pair per class) is not built")
        b, c, h, w = fmap.shape
        if wh.shape[1] != 2 or (reg is not None and reg.shape[1] != 2):
            raise ValueError("CenterNetDecoder.decode: wh and reg have two channels")
        if not 0 < K <= min(2048, h * w):
            raise ValueError(f"CenterNetDecoder.decode: K={K} must lie in 1..min(2048, H*W)")
        need_device_all((fmap, wh, reg), _MODULE)
        ld = round_up8(c)
        p = fmap.float()
        logits = _to_pm(torch.log(p) - torch.log1p(-p), ld)
        whp = _to_pm(wh.float(), 8)
        regp = _to_pm(reg.float(), 8) if reg is not None else None
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=fmap.device)
        boxes, scores = f(b, K, 4), f(b, K)
        classes = torch.empty((b, K), dtype=torch.int32, device=fmap.device)
        ws = torch.empty(ops.centernet_decode_workspace_bytes(b, c, h, w), dtype=torch.uint8, device=fmap.device)
        ops.centernet_decode(logits, ld, whp, 8, 0, regp, 8, 0, b, c, h, w, K, boxes, scores, classes, ws)
        return boxes, scores.reshape(b, K, 1), classes.float().reshape(b, K, 1)

    @staticmethod
    def transform_boxes(boxes, center, size, output_size, scale=1):
        """centernet.py:293-311 on the host: the affine map of three point pairs (cv2.getAffineTransform(dst, src)) solved with
        numpy.linalg, applied to the box corners."""
        if isinstance(boxes, torch.Tensor):
            boxes = boxes.detach().cpu().numpy()
        boxes = np.asarray(boxes).reshape(-1, 4)
        trans = CenterNetDecoder.affine_matrix(center, size, output_size)
        pts = boxes.reshape(-1, 2).astype(np.float64)
        return (pts @ trans[:, :2].T + trans[:, 2]).reshape(-1, 4)

    @staticmethod
    def affine_matrix(center, size, output_size):
        """The float64 (2, 3) map of transform_boxes: trans @ (x, y, 1) takes an output-map point to the source image."""
        src, dst = CenterNetDecoder.generate_src_and_dst(center, size, output_size)
        a = np.column_stack((np.float32(dst).astype(np.float64), np.ones(3)))
        return np.linalg.solve(a, np.float32(src).astype(np.float64)).T

    @staticmethod
    def pseudo_nms(fmap, pool_size=3):
        """centernet.py:313-325: keep the elements that equal the maximum of their pool_size window, zero the others."""
        need_device_all((fmap,), _MODULE)
        f = fmap.float()
        peak = TF.max_pool2d(f, pool_size, stride=1, padding=(pool_size - 1) // 2) == f
        return f * peak.float()

    @staticmethod
    def topk_score(scores, K=40):
        """centernet.py:327-352: the K best per class plane, then the K best of those per image -> (scores, pixel index, class, y, x),
        each (batch, K)."""
        need_device_all((scores,), _MODULE)
        b, c, h, w = scores.shape
        per_cls, pix = torch.topk(scores.reshape(b, c, h * w), K)
        best, pos = torch.topk(per_cls.reshape(b, c * K), K)
        pix = torch.gather(pix.reshape(b, c * K), 1, pos)
        return best, pix, (pos // K).to(torch.int32), (pix // w).float(), (pix % w).float()

    @staticmethod
    def generate_src_and_dst(center, size, output_size):
        """centernet.py:354-375: three points of the source square (its centre, the point half a side above it, and that point moved
        half a side to the left) and the same three of the output map, float32 (3, 2) each."""
        side = size[0] if np.ndim(size) else size        # a scalar is a square's side
        dst_w, dst_h = output_size

        def corners(c, width):
            half = width * -0.5
            pts = np.zeros((3, 2), dtype=np.float32)
            pts[0] = c
            pts[1] = pts[0].astype(np.float64) + (0.0, half)
            pts[2] = pts[1].astype(np.float64) + (half, 0.0)
            return pts
        return corners(center, side), corners((dst_w * 0.5, dst_h * 0.5), dst_w)


class CenterNetGT:
    """The per-image helpers of the reference on host numpy arrays (float32 where the reference's tensors are).  The batch path is
    centernet_ground_truth: one launch for all images."""

    @staticmethod
    def generate_score_map(fmap, gt_class, gt_wh, centers_int, min_overlap):
        """centernet.py:380-391: fmap (K, H, W) float32 array, changed in place and returned."""
        radius = CenterNetGT.get_gaussian_radius(gt_wh, min_overlap)
        radius = np.maximum(radius, 0).astype(np.int32)
        for i in range(len(gt_class)):
            c = int(gt_class[i])
            if c >= 0:
                fmap[c] = CenterNetGT.draw_gaussian(fmap[c], centers_int[i], int(radius[i]))
        return fmap

    @staticmethod
    def get_gaussian_radius(box_size, min_overlap):
        """centernet.py:393-423 (the "bug version"), float32, one rounding per operation, in the order written."""
        box = np.asarray(box_size, dtype=np.float32)
        if box.size == 0:
            return np.zeros((0,), np.float32)
        f = np.float32
        width, height = box[..., 0], box[..., 1]
        b1 = height + width
        c1 = width * height * f(1 - min_overlap) / f(1 + min_overlap)
        sq1 = np.sqrt(b1 * b1 - f(4) * c1)
        r1 = (b1 + sq1) / f(2)
        b2 = f(2) * (height + width)
        c2 = f(1 - min_overlap) * width * height
        sq2 = np.sqrt(b2 * b2 - f(16) * c2)
        r2 = (b2 + sq2) / f(2)
        b3 = f(-2 * min_overlap) * (height + width)
        c3 = f(min_overlap - 1) * width * height
        sq3 = np.sqrt(b3 * b3 - f(4 * (4 * min_overlap)) * c3)
        r3 = (b3 + sq3) / f(2)
        return np.minimum(np.minimum(r1, r2), r3)

    @staticmethod
    def gaussian2D(radius, sigma=1):
        """centernet.py:425-432: the (2m+1, 2n+1) float64 Gaussian window, values below eps * max cut to 0."""
        m, n = radius
        dy = np.arange(-m, m + 1).reshape(-1, 1)
        dx = np.arange(-n, n + 1).reshape(1, -1)
        g = np.exp(-(dx * dx + dy * dy) / (2 * sigma * sigma))
        g[g < np.finfo(g.dtype).eps * g.max()] = 0
        return g

    @staticmethod
    def draw_gaussian(fmap, center, radius, k=1):
        """centernet.py:434-452: fmap (H, W) <- max(fmap, k * window) over the part of the window that lies inside the map."""
        g = CenterNetGT.gaussian2D((radius, radius), sigma=(2 * radius + 1) / 6).astype(np.float32)
        cx, cy = int(center[0]), int(center[1])
        H, W = fmap.shape[:2]
        x0, x1 = cx - min(cx, radius), cx + min(W - cx, radius + 1)
        y0, y1 = cy - min(cy, radius), cy + min(H - cy, radius + 1)
        if x1 > x0 and y1 > y0:
            win = g[y0 - cy + radius:y1 - cy + radius, x0 - cx + radius:x1 - cx + radius]
            fmap[y0:y1, x0:x1] = np.maximum(fmap[y0:y1, x0:x1], win * k)
        return fmap


@registers.models.register()
class CenterNet(FPNDetector):
    """models/det/centernet.py:17-186 (module docstring: the seams, the arena, what stays layer-owned)."""

    HAS_FPN = False
    TOP_BLOCK = None
    BOTTOM_UP = "backbone"            # CenterNet holds the bare ResNet: backbone.conv1, backbone.layerL.B.* (no bottom_up, no fc)
    TOPK = 100                        # CenterNetDecoder.decode's default K

    @staticmethod
    def init_params(cfg, seed=0):
        """The backbone's parameters (models/cls/resnet.py's initialisers); the neck and head initialise themselves (layers/center_head.py)."""
        p = {}
        P.init_resnet(p, np.random.default_rng(seed), cfg.MODEL.BACKBONE.NAME, prefix="backbone")
        return p

    @classmethod
    def check_config(cls, cfg):
        from ..layers.center_head import validate_head, validate_neck
        m = cfg.MODEL
        if m.get("WEIGHT_DTYPE", "bf16") != "bf16":
            raise ValueError(f"MODEL.WEIGHT_DTYPE = {m.WEIGHT_DTYPE!r} is not supported by CenterNet: the fp8 paths of the neck and head are not built; use 'bf16'")
        if m.BACKBONE.NAME not in P.RESNET_SPECS:
            raise ValueError(f"MODEL.BACKBONE.NAME = {m.BACKBONE.NAME!r} is not supported: one of {sorted(P.RESNET_SPECS)}")
        super().check_config(cfg)
        h = m.HEAD
        ch, kern = list(h.DECONV_CHANNEL), list(h.DECONV_KERNEL)
        c5 = 512 * (4 if P.RESNET_SPECS[m.BACKBONE.NAME][0] == "bottleneck" else 1)
        if not ch or ch[0] != c5:
            raise ValueError(f"MODEL.HEAD.DECONV_CHANNEL[0] = {ch[:1]!r} must equal res5's channel count of {m.BACKBONE.NAME}, {c5}")
        if h.IN_CHANNELS != ch[-1]:
            raise ValueError(f"MODEL.HEAD.IN_CHANNELS = {h.IN_CHANNELS!r} must equal MODEL.HEAD.DECONV_CHANNEL[-1] = {ch[-1]}")
        if h.DOWN_SCALE != 32 / 2 ** len(kern):
            raise ValueError(f"MODEL.HEAD.DOWN_SCALE = {h.DOWN_SCALE!r} must be 32 / 2 ** len(MODEL.HEAD.DECONV_KERNEL) = {32 / 2 ** len(kern):g}")
        try:
            validate_neck(ch, kern)
        except ValueError as e:
            raise ValueError(f"MODEL.HEAD.DECONV_CHANNEL / DECONV_KERNEL: {e}") from e
        try:
            validate_head(h.IN_CHANNELS, cfg.DATA.NUM_CLASSES)
        except ValueError as e:
            raise ValueError(f"MODEL.HEAD.IN_CHANNELS / DATA.NUM_CLASSES: {e}") from e
        size = m.OUTPUT_SIZE
        if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and v > 0 for v in size)):
            raise ValueError(f"MODEL.OUTPUT_SIZE = {size!r} is not supported: (H, W), two positive integers")
        if not (isinstance(h.TENSOR_DIM, int) and 1 <= h.TENSOR_DIM <= 1024):
            raise ValueError(f"MODEL.HEAD.TENSOR_DIM = {h.TENSOR_DIM!r} is not supported: an integer from 1 to 1024 (bd_centernet_targets)")

    @staticmethod
    def param_shapes(cfg):
        """{state_dict name: shape} of the detector a config describes, without touching the device: backbone.* (the bare ResNet, no fc),
        upsample.deconvI.*, head.{cls,wh,reg}_head.*."""
        from ..layers.center_head import head_param_shapes, neck_param_shapes
        h = cfg.MODEL.HEAD
        out = {k: tuple(v.shape) for k, v in CenterNet.init_params(cfg).items()}
        out.update({"upsample." + k: tuple(v) for k, v in neck_param_shapes(list(h.DECONV_CHANNEL), bool(h.MODULATE_DEFORM)).items()})
        out.update({"head." + k: tuple(v) for k, v in head_param_shapes(h.IN_CHANNELS, cfg.DATA.NUM_CLASSES).items()})
        return out

    @classmethod
    def check_batch(cls, cfg, image_hw, gt_slots=None):
        """What only a training batch can tell, from host shapes alone: MODEL.OUTPUT_SIZE (the targets' map) = the padded input size /
        DOWN_SCALE, and the gt slots fit HEAD.TENSOR_DIM.  Inference reads neither key."""
        m = cfg.MODEL
        ds = m.HEAD.DOWN_SCALE
        hp, wp = (round_up32(v) for v in image_hw)
        want = (int(hp // ds), int(wp // ds))
        if tuple(m.OUTPUT_SIZE) != want:
            raise ValueError(f"MODEL.OUTPUT_SIZE = {tuple(m.OUTPUT_SIZE)!r} does not match this batch: the padded input {hp} x {wp} / "
                             f"HEAD.DOWN_SCALE {ds} gives (H, W) = {want}")
        if gt_slots is not None and gt_slots > m.HEAD.TENSOR_DIM:
            raise ValueError(f"MODEL.HEAD.TENSOR_DIM = {m.HEAD.TENSOR_DIM} is smaller than the batch's {gt_slots} gt slots")

    # ---- construction ----------------------------------------------------------------------------------------------------------------------
    def _build_head(self, add, params):
        from ..layers.center_head import CenterHead, CenternetDeconv
        m, h = self.cfg.MODEL, self.cfg.MODEL.HEAD
        self.neck = CenternetDeconv(list(h.DECONV_CHANNEL), list(h.DECONV_KERNEL), bool(h.MODULATE_DEFORM), device=self.device)
        self.head = CenterHead(h.IN_CHANNELS, self.num_classes, h.CLS_PRIOR_PROB, device=self.device)
        self.cls_ld = self.head.cls_ld
        self._adopted = AdoptedParts([("upsample", self.neck), ("head", self.head)], self.device)
        # the neck's norms are records of the model's LiveNorms: running statistics in norms.running (broadcast, EMA buffer average)
        self._neck_norms = {f"upsample.{n}.{b}": self.norms.add(f"upsample.{n}.{b}", l.out_planes) for n, l in self.neck.layers()
                            for b in l.NORMS}

    def _reserve_head(self, arena):
        """Neck, then head, behind the trunk: one contiguous "head" bucket.  Norm vectors sit right behind their convolution's slots."""
        for n, l in self.neck.layers():
            behind = {f"dcn.{l.dcn.DCN_NAME}.bias": "dcn_bn", "up_sample.weight": "up_bn"}
            for k in l.arena_shapes():
                self._adopted.reserve(arena, [f"upsample.{n}.{k}"])
                if k in behind:
                    self._neck_norms[f"upsample.{n}.{behind[k]}"].reserve(arena)
        self._adopted.reserve(arena, ["head." + k for k in self.head.arena_shapes()])

    def _finish_layers(self, params):
        self._adopted.adopt_onto(self.arena, self._neck_norms)
        self._post = {}
        super()._finish_layers(params)

    def _head_convs(self):
        return []

    def _head_wgrad_ws_bytes(self, pl):
        return 0           # (the neck and head own their workspaces)

    def _debug_head(self, pl, out, lvl):
        pass

    # ---- parameters --------------------------------------------------------------------------------------------------------------------------
    def _bind_params(self, params):
        """FPNDetector._bind_params for the trunk; the neck's and head's entries, when the dict has them (a backbone-only classification
        checkpoint does not: load_weights(strict=False) leaves them as they are), go in through the layers' strict load_state_dict."""
        self._adopted.bind(params)
        super()._bind_params({k: v for k, v in params.items() if k.startswith("backbone.")})

    def repack_weights(self):
        super().repack_weights()
        self._repack_head()

    def repack_trainable(self):
        super().repack_trainable()
        self._repack_head()

    def _repack_head(self):
        self._adopted.repack()
        if not self.training:
            self._adopted.refresh_eval()

    def train(self, mode=True):
        super().train(mode)
        self._adopted.train(mode)
        if not mode:
            self._adopted.refresh_eval()
        return self

    def state_dict(self):
        return {**super().state_dict(), **self._adopted.state_dict()}

    def reference_grads(self):
        return {**super().reference_grads(), **self._adopted.grads()}

    def reference_grads_names(self):
        return super().reference_grads_names() + self._adopted.grad_names()

    # ---- plan ----------------------------------------------------------------------------------------------------------------------------------
    def _plan_head(self, pl):
        """Targets, loss gradients and loss sums of one padded shape (the neck's and head's activations are layer-owned)."""
        C = pl._carve
        f32, bf = torch.float32, torch.bfloat16
        N, T, K = pl.N, int(self.cfg.MODEL.HEAD.TENSOR_DIM), self.num_classes
        g5 = pl.blk[-1].gout
        s = 2 ** self.neck.num_layers
        pl.H5, pl.W5 = g5.H[0], g5.W[0]
        pl.Ho, pl.Wo = s * pl.H5, s * pl.W5
        M = N * pl.Ho * pl.Wo
        pl.tgt = dict(score_map=C.empty((N, pl.Ho * pl.Wo, K), f32), wh=C.empty((N, T, 2), f32), reg=C.empty((N, T, 2), f32),
                      reg_mask=C.empty((N, T), f32), index=C.empty((N, T), torch.int32), num_pos=C.empty((1,), f32))
        pl.tgt_ws = C.empty((ops.centernet_targets_workspace_bytes(N),), torch.uint8)
        pl.d_logits = C.empty((M, self.cls_ld), bf)
        pl.d_wh, pl.d_reg, pl.d_wr = C.empty((M, 8), bf), C.empty((M, 8), bf), C.empty((M, 8), bf)
        pl.loss_buf = C.zeros((3,), f32)

    # ---- forward / losses ------------------------------------------------------------------------------------------------------------------
    def head_forward(self, pl):
        """res5's stored block output -> neck -> head, pixel-major bf16 all the way."""
        b5 = pl.blk[-1]
        pl.neck_in = b5.out
        pl.neck_out = self.neck.forward_pm(b5.out, pl.N, pl.H5, pl.W5)
        pl.logits, pl.wr = self.head.forward_pm(pl.neck_out, pl.N, pl.Ho, pl.Wo)

    @staticmethod
    def _host_shape(inputs):
        image = inputs["data"] if isinstance(inputs, dict) else inputs
        if hasattr(image, "Hmax"):
            return image.N, image.Hmax, image.Wmax
        return image.shape[0], image.shape[-2], image.shape[-1]

    def get_losses(self, inputs):
        """CenterNet.get_losses (centernet.py:129-155): one target launch, the focal loss and the two L1 losses with their gradients; the
        LOSS.* weights go in as the kernels' `weight`, so the gradients arrive weighted.  Device scalars, no host synchronisation."""
        assert self.training
        m = self.cfg.MODEL
        _, H, W = self._host_shape(inputs)
        self.check_batch(self.cfg, (H, W), inputs["gt_boxes"].shape[1])
        pre = self.pre_process(inputs)
        pl = pre["plan"]
        self._cur = pl
        gt = pre["gt_boxes"]
        num_gt = pre["img_info"][:, -1].to(torch.int32).contiguous()
        self.network_forward(pl)
        t, N, K, T = pl.tgt, pl.N, self.num_classes, int(m.HEAD.TENSOR_DIM)
        ops.centernet_targets_into(gt, num_gt, N, gt.shape[1], K, pl.Ho, pl.Wo, T, 1 / m.HEAD.DOWN_SCALE, m.HEAD.MIN_OVERLAP,
                                   t["score_map"], t["wh"], t["reg"], t["reg_mask"], t["index"], t["num_pos"], pl.tgt_ws)
        pl.loss_buf.zero_()
        ops.centernet_focal_fwd_bwd(pl.logits, t["score_map"], N * pl.Ho * pl.Wo, K, self.cls_ld, t["num_pos"], m.LOSS.CLS_WEIGHT, 1.0,
                                    pl.loss_buf[0:1], pl.d_logits)
        # (each L1 call writes all of its gradient buffer: two buffers, summed in head_backward)
        ops.centernet_l1_fwd_bwd(pl.wr, 8, 0, t["index"], t["reg_mask"], t["wh"], N, pl.Ho, pl.Wo, T, m.LOSS.WH_WEIGHT, 1.0,
                                 pl.loss_buf[1:2], pl.d_wh)
        ops.centernet_l1_fwd_bwd(pl.wr, 8, 2, t["index"], t["reg_mask"], t["reg"], N, pl.Ho, pl.Wo, T, m.LOSS.REG_WEIGHT, 1.0,
                                 pl.loss_buf[2:3], pl.d_reg)
        loss_cls, loss_wh, loss_reg = pl.loss_buf[0], pl.loss_buf[1], pl.loss_buf[2]
        return {"total_loss": loss_cls + loss_wh + loss_reg, "loss_cls": loss_cls, "loss_box_wh": loss_wh, "loss_center_reg": loss_reg}

    # ---- backward ----------------------------------------------------------------------------------------------------------------------------
    def head_backward(self, pl, ws, cws):
        """Head, then neck (their weight gradients on the main stream, into the arena), then the seam: the neck's d_x gated by res5's
        output is res5's g_out, dL/d(pre-activation)."""
        ops.add_bf16(pl.d_wh, pl.d_reg, pl.d_wr)
        g_f = self.head.backward_pm(pl.d_logits, pl.d_wr)
        pl.neck_dx = self.neck.backward_pm(g_f)
        b5 = pl.blk[-1]
        ops.relu_bwd_bf16(pl.neck_dx, b5.out, b5.g_out)

    # ---- inference -----------------------------------------------------------------------------------------------------------------------------
    def _affines(self, inputs, N, H, W, dst):
        """Per image the 2 x 3 map of CenterNet.post_process (centernet.py:175-178) as six float32 in dst [N][6], from the batch's
        im_info rows [pad_h, pad_w, origin_h, origin_w, ...] (absent: pre_process's default, the padded and the given size).
        Host im_info (the loaders'): float64 generate_src_and_dst + solve, rounded once, copied with the batch.  A device im_info is never
        read back: the same map in closed form -- the three point pairs differ by a scale s = pad_w / out_w on both axes, so
        a = e = s, b = d = 0, c = cx - s out_w / 2, f = cy - s out_h / 2 -- in float64 on the device, rounded once."""
        info = inputs.get("im_info") if isinstance(inputs, dict) else None
        ds = self.cfg.MODEL.HEAD.DOWN_SCALE
        if torch.is_tensor(info) and info.is_cuda:
            r = info.reshape(N, -1).double()
            s_h, s_w, o_h, o_w = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
            cx, cy = torch.floor(o_w / 2), torch.floor(o_h / 2)
            dw, dh = torch.floor(s_w / ds), torch.floor(s_h / ds)
            s = s_w / dw
            z = torch.zeros_like(s)
            dst.copy_(torch.stack([s, z, cx - s * dw / 2, z, s, cy - s * dh / 2], 1))
            return
        if info is None:
            info = np.asarray([[round_up32(H), round_up32(W), H, W]] * N, np.float64)
        else:
            info = (info.numpy() if torch.is_tensor(info) else np.asarray(info)).astype(np.float64).reshape(N, -1)[:, :4]
        out = np.empty((N, 6), np.float32)
        for i, row in enumerate(info):
            flipped = row[::-1]                                  # (origin_w, origin_h, pad_w, pad_h)
            out[i] = CenterNetDecoder.affine_matrix(flipped[:2] // 2, flipped[-2:], flipped[-2:] // ds).reshape(6)
        dst.copy_(torch.from_numpy(out), non_blocking=True)

    def inference_batch(self, inputs):
        """CenterNet.inference + post_process (centernet.py:157-186) for every image of the batch: decode on the raw head outputs, the
        boxes to image coordinates in one launch; a list of N Containers of TOPK rows each."""
        from ..structures import Boxes, Container
        assert not self.training
        N, H, W = self._host_shape(inputs)          # (any size: MODEL.OUTPUT_SIZE describes the training targets only)
        pre = self.pre_process(inputs)
        pl = self._cur = pre["plan"]          # (the plan whose head outputs this call leaves behind)
        self.network_forward(pl)
        K, k, dev = self.num_classes, self.TOPK, self.device
        sc = self._post.get((N, pl.Ho, pl.Wo))
        if sc is None:
            f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
            sc = self._post[(N, pl.Ho, pl.Wo)] = dict(
                boxes=f(N, k, 4), scores=f(N, k), classes=torch.empty((N, k), dtype=torch.int32, device=dev), aff=f(N, 6),
                ws=torch.empty(ops.centernet_decode_workspace_bytes(N, K, pl.Ho, pl.Wo), dtype=torch.uint8, device=dev))
        self._affines(inputs, N, H, W, sc["aff"])
        ops.centernet_decode(pl.logits, self.cls_ld, pl.wr, 8, 0, pl.wr, 8, 2, N, K, pl.Ho, pl.Wo, k, sc["boxes"], sc["scores"],
                             sc["classes"], sc["ws"])
        # (the results are the caller's: not part of the cached scratch)
        ob = torch.empty((N, k, 4), dtype=torch.float32, device=dev)
        osc = torch.empty((N, k), dtype=torch.float32, device=dev)
        ol = torch.empty((N, k), dtype=torch.int32, device=dev)
        ops.centernet_boxes_to_image(sc["boxes"], sc["aff"], sc["scores"], sc["classes"], N, k, ob, osc, ol)
        return [Container(boxes=Boxes(ob[i]), box_scores=osc[i], box_labels=ol[i]) for i in range(N)]
