"""RetinaNet (basedet/models/det/retinanet.py) on the HIP path: RetinaNetHead + anchor target assignment + focal / L1
losses on top of the shared ResNet-FPN trunk (fpn_base.py).

Same protocol as the reference's BaseNet (models/base_net.py:50-71): ``model(batch)`` in training mode returns
``{"total_loss", "cls_loss", "reg_loss"}``; the batch dict is the collator contract
(data/collators/pad_collator.py:38-49): ``data`` (N,3,H,W), ``gt_boxes`` (N,G,5), ``im_info`` (N,5).
"""
import torch

from .. import ops
from ..streams import fork, join
from ..utils.registry import registers
from . import params as P
from .engine import PaddedClsConv
from .fpn_base import FPNDetector, _round_up


@registers.models.register()
class RetinaNet(FPNDetector):
    READS_MATCHER = True        # MODEL.MATCHER.* (retinanet.py:33-37, :219); FreeAnchor's bag losses never call the matcher

    @staticmethod
    def init_params(cfg, seed=0):
        return P.init_retinanet_params(cfg, seed)

    @classmethod
    def check_config(cls, cfg):
        super().check_config(cfg)
        cls.check_anchor_config(cfg, matcher=cls.READS_MATCHER)
        if not cfg.MODEL.HEAD.get("WITH_NORM", True):
            # retina_head.py:54-61: WITH_NORM = False drops the towers' ReLUs, which this head does not implement
            raise ValueError("MODEL.HEAD.WITH_NORM = False is not supported for the RetinaNet family: only True (the default) is implemented")

    # ---- construction ------------------------------------------------------------------------------------
    def _build_head(self, add, params):
        """RetinaNetHead (layers/head/retina_head.py:9-70): two 4-conv towers + cls_score / bbox_pred, weights shared
        over the five levels."""
        m = self.cfg.MODEL
        ch = self.fpn_ch
        self.num_anchors = len(m.ANCHOR.SCALES[0]) * len(m.ANCHOR.RATIOS[0])
        nc = m.HEAD.NUM_CONVS
        self.cls_tower = [add(f"head.cls_subnet.{2 * i}", ch, ch, 3, 1, 1, bias=True) for i in range(nc)]
        self.box_tower = [add(f"head.bbox_subnet.{2 * i}", ch, ch, 3, 1, 1, bias=True) for i in range(nc)]
        A, K = self.num_anchors, self.num_classes
        # A groups of cls_ld = round_up(K, 8) channels (the identity for K % 8 == 0): any class count, 16-byte anchor rows
        self.cls_score = self.convs["head.cls_score"] = PaddedClsConv("head.cls_score", ch, A, K, 3, 1, 1, self.device)
        self.cls_ld = self.cls_score.cls_ld
        self.box_ld = _round_up(A * 4, 8)                                          # 36 -> 40 channels (8-aligned rows)
        self.bbox_pred = add("head.bbox_pred", ch, A * 4, 3, 1, 1, bias=True, cout_pad=self.box_ld)
        # MODEL.SPARSE_BOX_BWD (default on, bf16 only): the box branch's gradient is nonzero only around the foreground anchors (the
        # regression loss writes +0 elsewhere), so its backward launches skip the all-zero patches (bd_conv_desc.gskip: same bits).  The
        # class tower's focal gradient is dense and stays on the plain descriptors.
        if bool(m.get("SPARSE_BOX_BWD", True)) and m.get("WEIGHT_DTYPE", "bf16") == "bf16":
            for c in self.box_tower + [self.bbox_pred]:
                c.gskip = True
        # MODEL.SPARSE_BOX_CHAIN (default on): the liveness is handed down the box tower in maps carved beside the tower gradients (_plan_head)
        # instead of being scanned out of every gradient again -- by its data gradient AND its weight gradient (bd_conv_desc.gskip_gmap /
        # gskip_dxmap).  Off: every launch scans for itself, as before the maps existed.
        self.sparse_chain = bool(m.get("SPARSE_BOX_CHAIN", True))
        # MODEL.SPARSE_BOX_FWD (default on): the box tower's FORWARD convolutions compute only what the step reads.  The regression loss reads
        # bbox_pred's output at the foreground anchors alone, so the tower activation k layers below it is needed only within k pixels of
        # a foreground pixel -- by bbox_pred, by the ReLU gates and by the weight gradients of the sparse backward chain, whose gradients
        # vanish outside the same neighbourhoods.  bd_fwd_live_maps builds those sets from the labels under the backbone's forward pass;
        # the rest of every activation holds +0 (the same bits in losses, gradients and dL/dP).  Exactly this class (FreeAnchor's bag
        # loss reads every anchor's offsets), with the sparse backward, bf16, training mode; bbox_pred itself stays dense.
        self.sparse_box_fwd = (bool(m.get("SPARSE_BOX_FWD", True)) and type(self) is RetinaNet and nc >= 1 and nc <= 8
                               and all(c.gskip for c in self.box_tower + [self.bbox_pred]))
        self._build_base_anchors()

    def _head_convs(self):
        return self.cls_tower + self.box_tower + [self.cls_score, self.bbox_pred]

    def _plan_head(self, pl):
        ch = self.fpn_ch
        N = pl.N
        C = pl._carve
        bf = torch.bfloat16

        def act(g, c):
            return C.empty((g.pixels, c), bf)

        nc = len(self.cls_tower)
        pl.cls_act = [act(pl.pyr, ch) for _ in range(nc)]
        pl.box_act = [act(pl.pyr, ch) for _ in range(nc)]
        A, K = self.num_anchors, self.num_classes
        pl.logits = act(pl.pyr, A * self.cls_ld)       # (pad slots K..cls_ld-1 of every anchor: zero weight rows and bias -> logit 0)
        pl.offsets = act(pl.pyr, self.box_ld)          # (channels 36..39: zero weight rows and bias -- written as 0 by every forward)
        pl.d_logits = C.like(pl.logits)                # (the losses write the pad slots' zero gradient)
        pl.d_offsets = C.like(pl.offsets)              # (bd_smooth_l1_fwd_bwd writes the padding slots' zero gradient)
        pl.g_tower = [[act(pl.pyr, ch) for _ in range(nc)] for _ in range(2)]   # one gradient buffer per tower layer
        # one liveness map per BOX tower gradient (int32; the layout is the library's).  A plan's buffers never overlap each other (_Carver
        # hands out disjoint ranges), so within a plan only the tower's own data gradient writes g_tower[1][i]: the promise that it still holds
        # last step's layout (gskip_dx_clean) can be given while the arena's epoch stands -- see head_backward
        pl.g_map = None
        if self.sparse_chain and all(c.gskip for c in self.box_tower + [self.bbox_pred]):
            nb = ops.conv2d_gskip_map_bytes(self.box_tower[0].desc(pl.pyr, pl.pyr))
            if nb:
                pl.g_map = [C.empty(((nb + 3) // 4,), torch.int32) for _ in range(nc)]
        pl.chain_epoch = None
        # one forward liveness map per BOX tower activation (int32; the layout is the library's): box_act[i] is needed within nc - i pixels of
        # the foreground.  fwd_epoch: the arena epoch at which the last forward on this plan left box_act in a map's layout (None: it did
        # not) -- the promise of bd_conv_desc.fwd_clean stands under the same rule as the backward chain's
        pl.f_map = None
        if self.sparse_box_fwd:
            nb = ops.fwd_live_map_bytes(self.box_tower[0].desc(pl.pyr, pl.pyr))
            if nb:
                pl.f_map = [C.empty(((nb + 3) // 4,), torch.int32) for _ in range(nc)]
        pl.fwd_epoch = None
        pl.fwd_skip = None          # (clean,) between get_losses' map launch and the head_forward that consumes it
        pl.fwd_skipped = False      # the last head_forward on this plan skipped: box_act / offsets are not the dense tensors
        # fp8 forward: every tower activation gets an e4m3 twin, written by the launch that produces it (no cast passes in the head)
        tw = lambda: C.empty((pl.pyr.pixels, ch), torch.uint8)      # noqa: E731
        pl.cls_act8 = [tw() if c.fp8 else None for c in self.cls_tower]
        pl.box_act8 = [tw() if c.fp8 else None for c in self.box_tower]
        # fp8 data gradients: e5m2 twins of the tower gradients and of dL/dP, written by the launch that produces them
        tg = self.fp8_grad_twins
        pl.g_tower8 = [[tw() if (c.fp8_dgrad and tg) else None for c in tower] for tower in (self.cls_tower, self.box_tower)]
        pl.g_P8 = tw() if (tg and all(t[0].fp8_dgrad for t in (self.cls_tower, self.box_tower))) else None
        self._plan_anchors(pl)
        tot = pl.A_total
        pl.labels = C.empty((N, tot), torch.int32)
        pl.match_idx = C.empty((N, tot), torch.int32)
        pl.gt_offsets = C.empty((N, tot, 4), torch.float32)
        pl.num_fg = C.zeros((1,), torch.int32)
        pl.loss_buf = C.zeros((2,), torch.float32)

    # ---- forward -----------------------------------------------------------------------------------------
    def head_forward(self, pl):
        # head (retina_head.py:103-112), all five levels per launch
        # MODEL.HEAD_TOWERS_CONCURRENT (round 6, default on): the box tower on a second stream beside the class tower -- the two are independent
        # until the losses.  Each launch is a full persistent grid, so the second tower's workgroups start on a CU the moment the first tower's
        # finish there: what is recovered is the launch-level loss of a one-workgroup-per-CU kernel (dispatch, the XCDs' finish spread:
        # the 0.907 factor of profiles/r06_pp_power.txt), +0.4-0.5 % per step on three boxes (profiles/r06_head_towers_ab.txt).  The same on the
        # BACKWARD pass, where the weight-gradient stream already runs beside the chain, costs 1.2 %: not done.  Steps that keep the weight
        # gradients on the main stream (bench.py's instrumented steps, --serial-wgrad) stay serial here too: clean per-kernel durations.
        # (bf16 only: in fp8 mode the tower convolutions may share the main stream's cast scratch)
        # The second stream is the model's auxiliary stream (the target assignment at the start of the forward pass is long done here), not one
        # of its own: see SideStreams.
        concurrent = bool(self.cfg.MODEL.get("HEAD_TOWERS_CONCURRENT", True)) and self.weight_dtype != "fp8_e4m3"
        side = self.streams.aux() if concurrent else None
        # MODEL.SPARSE_BOX_FWD: get_losses left this step's liveness maps on the auxiliary stream; a box tower that runs on the main stream
        # instead waits for them here
        skip, pl.fwd_skip = pl.fwd_skip, None
        if skip is not None and side is None:
            join(self.streams.aux_stream)
        if skip is None:
            pl.fwd_epoch = None          # a dense forward: box_act is in no map's layout any more
        pl.fwd_skipped = skip is not None
        with fork(side):
            t, t8 = pl.P, getattr(pl, "P8", None)
            for i, (c, a, a8) in enumerate(zip(self.box_tower, pl.box_act, pl.box_act8)):
                if skip is not None:
                    c.forward(t, pl.pyr, pl.pyr, a, relu=True, fwd_map=pl.f_map[i], fwd_clean=skip[0])
                else:
                    c.forward(t, pl.pyr, pl.pyr, a, relu=True, x8=t8, y8=a8)
                t, t8 = a, a8
            self.bbox_pred.forward(t, pl.pyr, pl.pyr, pl.offsets, x8=t8)
        t, t8 = pl.P, getattr(pl, "P8", None)
        for c, a, a8 in zip(self.cls_tower, pl.cls_act, pl.cls_act8):
            c.forward(t, pl.pyr, pl.pyr, a, relu=True, x8=t8, y8=a8); t, t8 = a, a8
        self.cls_score.forward(t, pl.pyr, pl.pyr, pl.logits, x8=t8)
        join(side)

    def get_losses(self, inputs):
        """RetinaNet.get_losses (retinanet.py:120-170)."""
        assert self.training
        pre = self.pre_process(inputs)
        pl = pre["plan"]
        self._cur = pl
        m = self.cfg.MODEL
        gt = pre["gt_boxes"]
        num_gt = pre["img_info"][:, 4].to(torch.int32).contiguous()
        N, Gmax = gt.shape[0], gt.shape[1]
        ws = self._scratch("assign", N * Gmax * 4).view(torch.float32)     # (N x Gmax floats: grows with the batch's Gmax, not the shape)
        thr = m.MATCHER.THRESHOLDS
        # The target assignment depends on the anchors and the gt boxes only (retinanet.py:211-232), not on the network's output: its two
        # launches (~0.12 ms at 16 x 201 600 anchors) run on the auxiliary stream under the forward pass instead of between forward and losses.
        side = self.streams.aux() if m.get("ASSIGN_ON_SIDE_STREAM", True) else None
        with fork(side):
            ops.retina_assign_encode(pl.anchors, gt, num_gt, thr[0], thr[1], m.MATCHER.ALLOW_LOW_QUALITY, m.BOX_REG.MEAN,
                                     m.BOX_REG.STD, pl.labels, pl.match_idx, pl.gt_offsets, pl.num_fg, ws)
            if pl.f_map is not None and self.streams.aux() is not None:
                # the box tower's forward liveness, right behind the assignment that wrote the labels: maps[k - 1] belongs to the activation
                # k layers below bbox_pred.  The promise that box_act still holds the previous step's layout: as head_backward's.
                # Only with the side streams on: a serial step (async_wgrad off: bench.py's instrumented steps, the per-element launch
                # audits) keeps every launch dense -- whole output tensors and clean per-kernel durations, and no map launch in the
                # main stream's way
                clean = pl.fwd_epoch == self.plan_arena.epoch
                pl.fwd_epoch = self.plan_arena.epoch
                ops.fwd_live_maps(self.box_tower[0].desc(pl.pyr, pl.pyr), pl.labels, self.num_anchors, pl.f_map[::-1], reset=not clean)
                pl.fwd_skip = (clean,)
        self.network_forward(pl)
        join(side)
        pl.loss_buf.zero_()
        rows = N * pl.A_total
        ops.focal_loss_fwd_bwd(pl.logits, pl.labels, rows, self.num_classes, m.LOSSES.FOCAL_LOSS_ALPHA,
                               m.LOSSES.FOCAL_LOSS_GAMMA, pl.num_fg, 1.0, pl.loss_buf[0:1], pl.d_logits, ld=self.cls_ld)
        ops.smooth_l1_fwd_bwd(pl.offsets, pl.gt_offsets, pl.labels, pl.pyr.pixels, self.num_anchors, self.box_ld,
                              m.LOSSES.SMOOTH_L1_BETA, pl.num_fg, m.LOSSES.REG_LOSS_WEIGHT, pl.loss_buf[1:2], pl.d_offsets)
        cls_loss, reg_loss = pl.loss_buf[0], pl.loss_buf[1]
        return {"total_loss": cls_loss + reg_loss, "cls_loss": cls_loss, "reg_loss": reg_loss}

    # ---- backward ----------------------------------------------------------------------------------------
    def head_backward(self, pl, ws, cws):
        pyr = pl.pyr
        # ---- head: cls tower then box tower; both end in g_P.  g_tower[t][i] = dL/d(pre-activation of tower conv i)
        # fp8 mode: a tower gradient's e5m2 twin g8[i] is written by the data-gradient launch that produces it and read by the next
        # one (no cast passes inside a tower); a twin is valid only if its producer writes one (the 40-channel box regressor does not)
        for ti, (tower, acts, pred, dpred) in enumerate(((self.cls_tower, pl.cls_act, self.cls_score, pl.d_logits),
                                                         (self.box_tower, pl.box_act, self.bbox_pred, pl.d_offsets))):
            gbuf, g8 = pl.g_tower[ti], pl.g_tower8[ti]
            n = len(tower)
            # box tower: the liveness maps travel down the chain -- bbox_pred's data gradient scans d_offsets (40 channels) and leaves the map
            # of gbuf[n - 1]; every layer below reads the map of its gradient (data and weight gradient: no scan) and leaves the next one.
            # The promise that a gradient buffer still holds last step's layout stands only if that step ran this chain on this plan and
            # nothing re-bound, grew or re-based the arena since (PlanArena.epoch); any other step withdraws it.
            maps = pl.g_map if (ti == 1 and self.sparse_chain and all(c.gskip for c in tower + [pred])) else None
            if ti == 1:
                clean = maps is not None and pl.chain_epoch == self.plan_arena.epoch
                pl.chain_epoch = self.plan_arena.epoch if maps is not None else None
                if maps is not None:
                    pred.set_chain(None, maps[n - 1], clean)
                    for i in range(n):
                        tower[i].set_chain(maps[i], maps[i - 1] if i > 0 else None, clean)
            gs = tower[n - 1].grad_scale
            self._wgrad(pred, acts[-1], dpred, pyr, pyr, ws, cws)
            tw = g8[n - 1] if pred.dgrad_writes_twin(pyr, pyr) else None       # None also when twins are off (g8 holds no buffers)
            if not pred.dgrad(dpred, pyr, pyr, gbuf[n - 1], mask=acts[-1], dx8=tw, q_scale=gs):
                tw = None
            act8 = pl.cls_act8 if ti == 0 else pl.box_act8
            for i in range(n - 1, -1, -1):
                x = acts[i - 1] if i > 0 else pl.P
                # the weight gradient reads the same twins: the tower input's (forward) and the gradient's (tw: written with gbuf[i])
                x8 = (act8[i - 1] if i > 0 else pl.P8) if tw is not None else None
                self._wgrad(tower[i], x, gbuf[i], pyr, pyr, ws, cws, x8=x8, g8=tw)
                if i > 0:
                    nxt = g8[i - 1] if tower[i].dgrad_writes_twin(pyr, pyr) else None
                    wrote = tower[i].dgrad(gbuf[i], pyr, pyr, gbuf[i - 1], mask=acts[i - 1], g8=tw, dx8=nxt, q_scale=tower[i - 1].grad_scale)
                    tw = nxt if wrote else None
                else:
                    # dL/dP's twin goes to the FPN output convolutions: THEIR scale (another scale group)
                    wrote_p = tower[i].dgrad(gbuf[i], pyr, pyr, pl.g_P, first=(ti == 0), g8=tw,
                                             dx8=pl.g_P8 if tower[i].dgrad_writes_twin(pyr, pyr) else None,
                                             q_scale=self.output[self.fpn_stages[0]].grad_scale)
        for c in self.box_tower + [self.bbox_pred]:
            c.set_chain()
        # the box tower's launch wrote the twin of the FINAL dL/dP (it accumulates onto the class tower's contribution)
        pl.g_P8_ready = pl.g_P8 is not None and bool(wrote_p)

    def _debug_head(self, pl, out, lvl):
        """The head's stored activations.  When the last forward skipped (MODEL.SPARSE_BOX_FWD), box_act and offsets hold +0 outside the
        foreground's reach: the box tower and bbox_pred are first run again densely from pl.P into the same buffers -- WITH THE CURRENT
        WEIGHTS (call this before an optimizer step to see the forward's own values) -- and the promise about box_act is withdrawn."""
        if getattr(pl, "fwd_skipped", False):
            t = pl.P
            for c, a in zip(self.box_tower, pl.box_act):
                c.forward(t, pl.pyr, pl.pyr, a, relu=True); t = a
            self.bbox_pred.forward(t, pl.pyr, pl.pyr, pl.offsets)
            pl.fwd_skipped = False
            pl.fwd_epoch = None
        for i in range(pl.pyr.nlev):
            for k in range(len(self.cls_tower)):
                out[f"cls{k}_{i}"] = lvl(pl.cls_act[k], i)
                out[f"box{k}_{i}"] = lvl(pl.box_act[k], i)
            lg = lvl(pl.logits, i)
            out[f"logits_{i}"] = self.cls_score.real_logits(lg.permute(0, 2, 3, 1)).permute(0, 3, 1, 2).contiguous()
            out[f"offs_{i}"] = lvl(pl.offsets, i, self.num_anchors * 4)

    # ------------------------------------------------------------------------------------------------
    # inference (retinanet.py:172-201) -- the reference takes one image; here N images of one padded shape share every launch
    # ------------------------------------------------------------------------------------------------
    def inference_batch(self, inputs):
        """The detections of every image of the batch: a list of N Containers (FPNDetector.inference unwraps a single one)."""
        assert not self.training
        pre = self.pre_process(inputs)
        pl = pre["plan"]
        self.network_forward(pl)
        K, A = self.num_classes, self.num_anchors
        m = self.cfg.MODEL
        # F.sigmoid(F.flatten(logits)) (:184) happens inside the selection: no score tensor
        return self._detect(pl.N, [h * w * A for h, w in pl.sizes], K, 0, pre["img_info"], logits=pl.logits, anchors=pl.anchors,
                            offsets=pl.offsets, off_ld=self.box_ld, A=A, mean=m.BOX_REG.MEAN, std=m.BOX_REG.STD, cls_ld=self.cls_ld)
