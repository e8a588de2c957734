"""models.yolox.YOLOX, the YOLOX detector (models/det/yolox.py:17-148): layers.YOLOPAFPN on layers.CSPDarknet and
layers.YOLOXHead adopt()ed onto one parameter arena and one LiveNorms, the multi-scale pre_process, get_losses / backward for
Solver.minimize and inference from an image batch.  The kernels' glue -- assignment, losses, the inference chain -- is models/yolox.py's,
which re-exports the class; it is kept in this module, imported by its absolute name, so that the alias package's `basedet.models.yolox`
and `basedet_amd.models.yolox` hold one class."""
import numpy as np
import torch

from basedet_amd import ops
from basedet_amd.layers import yolox_blocks as B
from basedet_amd.layers._pm import round_up32
from basedet_amd.layers.yolox_head import head_param_shapes, validate_conv
from basedet_amd.models.adopted import AdoptedParts
from basedet_amd.models.engine import HostToDevice, ParamArena
from basedet_amd.models.live_norm import LiveNorms
from basedet_amd.utils.registry import registers

__all__ = ["YOLOX"]


def _glue():
    """models/yolox.py (imported late: it imports this module)."""
    from basedet_amd.models import yolox
    return yolox


@registers.models.register()
class YOLOX:
    """models/det/yolox.py:17-148: layers.YOLOPAFPN on layers.CSPDarknet -> layers.YOLOXHead, the losses and the inference chain of this
    module.  A stand-alone class (FPNDetector is a ResNet trunk) that provides what Solver, GradClip, ModelEMA, GradBuckets,
    broadcast_parameters and the checkpoint code read of a model.

    One parameter arena and one LiveNorms (the layers' adopt()): all convolution weights first -- backbone, PAFPN, head, the predictors'
    padded weights last -- then every 1-D parameter: the norms' gamma / beta in the same order, then the predictor biases.  `decay_end`
    is the element offset where the second part begins: YOLOXSolver decays [0, decay_end) only.  The pad rows of the predictors and
    Focus's four pad columns are zero, receive a zero gradient and so stay zero under any of the optimizer launches.  Activations and
    workspaces stay layer-owned; no plan arena, no weight-gradient side stream, one gradient bucket ("all")."""

    STRIDES = (8, 16, 32)
    MAX_CELLS = 64                       # bd_spp_* holds planes up to 64 x 64: the stride-32 map of a 2048 x 2048 input
    TOPK = 1000                          # yolox.py:129
    weight_dtype = "bf16"

    @classmethod
    def check_config(cls, cfg):
        m = cfg.MODEL
        if m.get("WEIGHT_DTYPE", "bf16") != "bf16":
            raise ValueError(f"MODEL.WEIGHT_DTYPE = {m.WEIGHT_DTYPE!r} is not supported by YOLOX: the fp8 paths of its layers are not built; use 'bf16'")
        if m.DEPTHWISE:
            raise ValueError(f"MODEL.DEPTHWISE = {m.DEPTHWISE!r} is not supported: DepthwiseConvBlock is not built")
        if m.ACTIVATION != "silu":
            raise ValueError(f"MODEL.ACTIVATION = {m.ACTIVATION!r} is not supported: the fused norm kernels are SiLU's")
        if m.BACKBONE.NAME != "csp_darknet":
            raise ValueError(f"MODEL.BACKBONE.NAME = {m.BACKBONE.NAME!r} is not supported: 'csp_darknet' (YOLOFPN / Darknet are not built)")
        if list(m.BACKBONE.OUT_FEATURES) != ["dark3", "dark4", "dark5"]:
            raise ValueError(f"MODEL.BACKBONE.OUT_FEATURES = {list(m.BACKBONE.OUT_FEATURES)!r} is not supported: ['dark3', 'dark4', 'dark5']")
        cls._check_size("AUG.TRAIN_SETTING.INPUT_SIZE", cfg.AUG.TRAIN_SETTING.INPUT_SIZE)
        try:          # every channel count the two factors give, before a layer touches the device
            B._validate(B.pafpn_convs(B.darknet_convs(m.DEPTH_FACTOR, m.WIDTH_FACTOR), m.DEPTH_FACTOR, m.WIDTH_FACTOR, (256, 512, 1024)))
            in_ch, mid = cls._head_channels(cfg)
            for c in in_ch:
                validate_conv(c, mid, 1, 1)
            validate_conv(mid, mid, 3, 1)
        except ValueError as e:
            raise ValueError(f"MODEL.DEPTH_FACTOR / WIDTH_FACTOR = {m.DEPTH_FACTOR!r} / {m.WIDTH_FACTOR!r}: {e}") from e

    @classmethod
    def _check_size(cls, key, size):
        ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and v > 0 and v % 32 == 0 for v in size)
        if not ok or max(size) > 32 * cls.MAX_CELLS:
            raise ValueError(f"{key} = {size!r} is not supported: (H, W), two positive multiples of 32 up to {32 * cls.MAX_CELLS} "
                             f"(bd_spp_fwd holds {cls.MAX_CELLS} x {cls.MAX_CELLS} cells at stride 32)")

    @staticmethod
    def _head_channels(cfg):
        w = cfg.MODEL.WIDTH_FACTOR
        return [int(c * w) for c in (256, 512, 1024)], int(256 * w)

    @staticmethod
    def param_shapes(cfg):
        """{state_dict name: shape} of the detector a config describes, without touching the device: backbone.backbone.* (CSPDarknet),
        backbone.* (PAFPN), head.*."""
        m = cfg.MODEL
        in_ch, mid = YOLOX._head_channels(cfg)
        out = {"backbone." + k: tuple(v) for k, v in B.pafpn_param_shapes(m.DEPTH_FACTOR, m.WIDTH_FACTOR).items()}
        out.update({"head." + k: tuple(v) for k, v in head_param_shapes(int(cfg.DATA.NUM_CLASSES), in_ch, mid).items()})
        return out

    # ---- construction ----------------------------------------------------------------------------------------------------------------------
    def __init__(self, cfg, params=None, device="cuda", seed=0):
        from basedet_amd.layers import CSPDarknet, YOLOPAFPN, YOLOXHead
        self.check_config(cfg)
        self.cfg, self.device, m = cfg, torch.device(device), cfg.MODEL
        self.training, self.use_l1 = True, False
        self.num_classes, self.strides = int(cfg.DATA.NUM_CLASSES), list(self.STRIDES)
        self.img_mean, self.img_std = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]          # (yolox.py:71-98 normalises nothing)
        d, w = m.DEPTH_FACTOR, m.WIDTH_FACTOR
        in_ch, mid = self._head_channels(cfg)
        bottom_up = CSPDarknet(d, w, out_features=tuple(m.BACKBONE.OUT_FEATURES), seed=seed, device=device)
        self.backbone = YOLOPAFPN(bottom_up, depth=d, width=w, seed=seed + 1000, device=device)
        self.head = YOLOXHead(self.num_classes, in_channels=in_ch, mid_channels=mid, seed=seed + 2000, device=device)
        self._parts = AdoptedParts([("backbone", self.backbone), ("head", self.head)], self.device)
        for _, c in self._norm_layers():                     # set_model_hyperparam (yolox.py:65-69); BN_MOMENTUM is MegEngine's convention
            c.eps = c.norm.eps = float(m.BN_EPS)
            c.momentum = c.norm.momentum = 1.0 - float(m.BN_MOMENTUM)
        self._build_arena()
        self._target_size = tuple(cfg.AUG.TRAIN_SETTING.INPUT_SIZE)
        self._h2d = HostToDevice(self.device, cfg)                 # (bd_h2d_submit: the one host-to-device route of the project)
        self._halo, self._pts, self._post = {}, {}, {}             # per shape: the input image, the points, the inference scratch
        self._cur = None
        self._pack_table = None
        self.extra_meter = {}
        if params is not None:
            self._bind_params(params)

    def _norm_layers(self):
        """[(state_dict prefix, ConvBNSiLU)] in forward order: backbone, PAFPN, head."""
        return [(n, c) for n, c in self._parts._leaves() if c.NORMS]

    def _build_arena(self):
        a = self.arena = ParamArena(self.device)
        self.norms = LiveNorms(self.device)
        shapes = self._parts.arena_shapes()
        self._parts.reserve(a, [k for k, shape in shapes.items() if len(shape) == 4])
        self.decay_end = a.total
        recs = {}
        for n, c in self._norm_layers():
            recs[n + ".norm"] = self.norms.add(n + ".norm", c.cout)
            recs[n + ".norm"].reserve(a)
        self._parts.reserve(a, [k for k, shape in shapes.items() if len(shape) == 1])
        a.allocate()
        self.norms.allocate()
        self._parts.adopt_onto(a, recs)

    def grad_buckets(self):
        """{phase: (lo, hi)} for GradBuckets: one bucket, closed at the end of backward()."""
        return {"all": (0, self.arena.total)}

    target_size = property(lambda self: self._target_size)

    @target_size.setter
    def target_size(self, size):
        """(H, W) of the next training batches (SyncSizeHook sets it): pre_process resizes a batch of another size to it."""
        size = tuple(int(v) for v in size) if isinstance(size, (tuple, list)) else size
        self._check_size("target_size", size)
        self._target_size = size

    # ---- parameters --------------------------------------------------------------------------------------------------------------------------
    def _bind_params(self, params):
        """(Re)load from a reference-layout dict (AdoptedParts.bind: strict per part, in place)."""
        self._parts.bind(params)
        if not self.training:
            self._fold_norms()

    def load_weights(self, weights, strict=False):
        from basedet_amd.utils.checkpoint import load_matched_weights
        return load_matched_weights(self, weights, strict)

    def load_state_dict(self, states, strict=True):
        return self.load_weights(states, strict=strict)

    def state_dict(self):
        return self._parts.state_dict()

    def repack_weights(self):
        self._parts.repack()
        if not self.training:
            self._fold_norms()

    def repack_trainable(self):
        """Every bf16 operand from its fp32 master in ONE launch (bd_weight_pack_multi); the table holds raw pointers into the arena and
        the packed tensors, which never move after construction."""
        if self._pack_table is None:
            self._pack_table = ops.build_pack_table([c.pack_entry() for _, c in self._parts._leaves()], self.device)
        ops.weight_pack_multi(self._pack_table)
        if not self.training:
            self._fold_norms()

    def _fold_norms(self, pack=True):
        """Evaluation reads 1 / sqrt(running_var + eps) of every norm, computed once here (the layers' refresh_eval)."""
        self._parts.refresh_eval()

    def train(self, mode=True):
        self.training = bool(mode)
        self._parts.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def reference_grads(self):
        return self._parts.grads()

    def reference_grads_names(self):
        return self._parts.grad_names()

    def state_dict_trainable_names(self):
        return list(self.reference_grads_names())

    def trainable_parameter_names(self):
        return [e[0] for e in self.arena.entries]

    # ---- forward -------------------------------------------------------------------------------------------------------------------------------
    def pre_process(self, inputs):
        """yolox.py:71-98.  The loader's fp32 (N, 3, H, W) batch, host or device -> x_halo bf16 (N, Hp + 6, Wp + 8, 4) with mean 0 and std
        1.  Training: a batch whose (H, W) is not target_size is resized to it bilinearly in the launch that writes x_halo
        (bd_resize_bilinear_normalize: no fp32 intermediate image) and the gt x / y are scaled by scale_w / scale_h.  Evaluation: the
        batch is only padded to a multiple of 32.  Returns {x_halo, N, H, W (of x_halo's image area), img_info[, gt_boxes]}."""
        image = inputs["data"] if isinstance(inputs, dict) else inputs
        if not (torch.is_tensor(image) and image.is_cuda):
            image = self._h2d(image)
        image = image.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        N, C, H, W = image.shape
        if C != 3:
            raise ValueError(f"YOLOX: the batch has {C} channels, expected (N, 3, H, W)")
        out = {"N": N}
        resize = self.training and (H, W) != tuple(self._target_size)
        if resize:
            h, w = self._target_size
            Hp, Wp = h, w
        else:
            h, w = H, W
            Hp, Wp = round_up32(H), round_up32(W)
            self._check_size("the padded batch size", (Hp, Wp))
        x_halo = self._halo.get((N, Hp, Wp))
        if x_halo is None:
            x_halo = self._halo[(N, Hp, Wp)] = torch.empty((N, Hp + 6, Wp + 8, 4), dtype=torch.bfloat16, device=self.device)
        if resize:
            ops.resize_bilinear_normalize(image, h, w, Hp, Wp, self.img_mean, self.img_std, x_halo)
        else:
            ops.pad_normalize(image, Hp, Wp, self.img_mean, self.img_std, x_halo)
        out.update(x_halo=x_halo, H=Hp, W=Wp)
        if self.training and isinstance(inputs, dict) and "gt_boxes" in inputs:
            gt = inputs["gt_boxes"]
            gt = (gt if torch.is_tensor(gt) else torch.as_tensor(np.asarray(gt))).to(self.device, dtype=torch.float32)
            if gt.shape[1] == 0:          # (a batch without an annotation: one all-zero row keeps the assignment's Gmax > 0 contract)
                gt = torch.zeros((gt.shape[0], 1, 5), dtype=torch.float32, device=self.device)
            if resize:
                gt = gt.clone()
                gt[..., 0:4:2] *= w / W
                gt[..., 1:4:2] *= h / H
            out["gt_boxes"] = gt.contiguous()
        if isinstance(inputs, dict) and "im_info" in inputs:
            info = inputs["im_info"]
            info = info if torch.is_tensor(info) else torch.as_tensor(np.asarray(info), dtype=torch.float32)
        else:
            info = torch.tensor([[h, w, h, w]] * N, dtype=torch.float32)          # (yolox.py:91-93)
        out["img_info"] = info.to(self.device, dtype=torch.float32).reshape(N, -1).contiguous()
        return out

    def network_forward(self, pre):
        """The PAFPN on pixel-major bf16: (the three levels' features, their sizes); the head follows in get_losses / inference_batch."""
        feats, sizes = self.backbone.forward_pm(pre["x_halo"], pre["N"], pre["H"], pre["W"])
        self._feats = list(feats)
        return self._feats, sizes

    def _points_of(self, sizes):
        key = tuple(sizes)
        if key not in self._pts:
            self._pts[key] = _glue()._points(sizes, self.strides, self.device)
        return self._pts[key]

    def get_losses(self, inputs):
        """yolox.py:150-265: pre_process, then the body of yolox_network_step up to the loss launch on the adopted layers; backward()
        runs the rest.  Device scalars, no host synchronisation."""
        assert self.training
        if not (isinstance(inputs, dict) and "gt_boxes" in inputs and "im_info" in inputs):
            raise ValueError("YOLOX.get_losses: the batch needs 'gt_boxes' and 'im_info' (the gt count is im_info's last column)")
        pre = self.pre_process(inputs)
        num_gt = pre["img_info"][:, -1].to(torch.int32).contiguous()
        feats, sizes = self.network_forward(pre)
        parts, d_cls, d_box_obj, assigned = _glue()._head_losses(self.head, feats, pre["N"], sizes, pre["gt_boxes"], num_gt, self.strides,
                                                                 self.use_l1, self._points_of(sizes))
        self._cur = dict(pre, parts=parts, d_cls=d_cls, d_box_obj=d_box_obj, assigned=assigned, sizes=sizes)
        return {"total_loss": parts.sum(), "iou_loss": parts[0], "l1_loss": parts[3], "obj_loss": parts[1], "cls_loss": parts[2]}

    def backward(self, on_bucket_ready=None):
        """Head, then PAFPN and backbone, their parameter gradients written (not added) into the arena's g views on the main stream."""
        assert self.training and self._cur is not None and "d_cls" in self._cur, "backward() needs a get_losses() before it"
        cur = self._cur
        d_feats = self.head.backward_pm(cur["d_cls"], cur["d_box_obj"], accumulate=False)
        self.backbone.backward_pm(d_feats, accumulate=False)
        if on_bucket_ready is not None:
            on_bucket_ready("all")

    def __call__(self, inputs):
        return self.forward(inputs)

    def forward(self, inputs):
        if self.training:
            return self.get_losses(inputs)
        return self.inference(inputs)

    # ---- inference -----------------------------------------------------------------------------------------------------------------------------
    def inference_batch(self, inputs):
        """yolox.py:107-148 for every image of the batch: an eval forward, then the head's own cls / box_obj through the chain
        yolox_inference runs behind its pack.  A list of N Containers; the scratch is cached per shape, the results are the caller's."""
        assert not self.training
        pre = self.pre_process(inputs)
        feats, sizes = self.network_forward(pre)
        cls, box_obj = self.head.forward_pm(feats, pre["N"], sizes)
        self._cur = dict(pre, sizes=sizes, cls=cls, box_obj=box_obj)
        return _glue()._detect_packed(cls, box_obj, self.num_classes, sizes, pre["img_info"], self.cfg, self.strides, self.TOPK,
                                      cache=self._post)

    def inference(self, inputs):
        """One image: its Container; a batch: the list of Containers in batch order."""
        outs = self.inference_batch(inputs)
        return outs[0] if len(outs) == 1 else outs
