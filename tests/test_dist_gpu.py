"""The data-parallel path on the GPU, through the bd_comm_* C ABI (RCCL).

One GPU: a communicator of a single rank sends every gradient bucket through RCCL on the communication stream (a SUM over one
rank is the identity, the MEAN scale is 1).  The parameters after three training steps must be bit-identical to a run without a
communicator: any missing dependency between the producing streams (main, weight-gradient side stream), the communication stream and
the SGD launch would show up as a stale or half-written gradient.

Two GPUs (skipped when the box has one): two ranks train three RetinaNet steps on DIFFERENT batches.  Both ranks must end with
bit-identical parameters, and those must equal a one-rank run on the concatenated batch up to fp32 summation order (the reference's
semantics: MEAN all-reduce of the gradients, lr = BASIC_LR * BATCHSIZE * world, solver/default_solver.py:99-124; both ranks hold the
same DummyLoader boxes, so the per-rank num_fg normalisers agree and the two runs compute the same mathematical update).

Each run is its own process (one process per GPU; nothing leaks into the other tests)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1])
out_path = sys.argv[2]
import numpy as np, torch
import basedet_amd
from basedet_amd import comm as bdcomm
world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
if world > 1 or os.environ.get("BD_FORCE_ALLREDUCE") == "1":
    bdcomm.set_comm(bdcomm.Comm.from_env())
from basedet_amd.configs import FCOSConfig, RetinaNetConfig
from basedet_amd.models import FCOS, RetinaNet, params as P
from basedet_amd.solver import DetSolver, broadcast_parameters
from basedet_amd.utils import DummyLoader
per_rank = int(os.environ["BD_TEST_BATCH"]) // world
fcos = os.environ.get("BD_TEST_MODEL", "retinanet") == "fcos"
cfg = FCOSConfig() if fcos else RetinaNetConfig()
cfg.MODEL.BATCHSIZE = per_rank
if os.environ.get("BD_TEST_WIRE"):
    cfg.SOLVER.ALLREDUCE_DTYPE = os.environ["BD_TEST_WIRE"]
if fcos:
    params = P.init_fcos_params(cfg, seed=0, residual_gamma=0.2)
    params["head.bbox_pred.bias"] = np.full_like(params["head.bbox_pred.bias"], 0.5)
    model = FCOS(cfg, params=params)
else:
    params = P.init_retinanet_params(cfg, seed=0, residual_gamma=0.2)
    model = RetinaNet(cfg, params=params)
if world > 1 and rank > 0:
    model.arena.w.add_(1.0)                      # rank 0's parameters must win (configs/detection_cfg.py:80-82)
    broadcast_parameters(model)
elif world > 1:
    broadcast_parameters(model)
solver = DetSolver.build(cfg, model)
assert solver.buckets.enabled == (bdcomm.get_comm() is not None)
assert abs(solver.optimizer.param_groups[0]["lr"] - cfg.SOLVER.BASIC_LR * per_rank * world) < 1e-12
solver.optimizer.param_groups[0]["lr"] = 1e-3
# the global batch: images of loaders seeded 0 and 1; a rank takes its contiguous slice (SURVEY 8e partitioning)
parts = [next(DummyLoader(2, (320, 448), seed=s)) for s in range(int(os.environ["BD_TEST_BATCH"]) // 2)]
full = {k: np.concatenate([np.asarray(p[k], dtype=np.float32) for p in parts], 0) for k in ("data", "gt_boxes", "im_info")}
if fcos:
    # the second half of the global batch (rank 1's slice when world = 2) keeps fewer gts: the ranks see DIFFERENT num_fg / sum ctr,
    # which FCOS averages over the ranks before normalising (models/det/fcos.py:143-144) -- then the mean of the per-rank gradients
    # equals the one-rank gradient on the concatenated batch
    half = full["im_info"].shape[0] // 2
    full["im_info"][half:, 4] = np.minimum(full["im_info"][half:, 4], [3, 2] * (half // 2) if half >= 2 else [3])
lo = rank * per_rank
batch = {k: torch.from_numpy(v[lo:lo + per_rank]).cuda() for k, v in full.items()}
if os.environ.get("BD_TEST_HOST_BATCH") == "1":
    # the loaders' form (DummyLoader / the collator yield numpy): the images go through bd_h2d_submit's staging threads, which must
    # bind to THIS rank's device and leave the process's current device alone (round-3 ADVICE: every rank staged to device 0)
    batch = dict(batch, data=np.ascontiguousarray(full["data"][lo:lo + per_rank]).astype(np.float64))
w0 = model.arena.w.clone()
for _ in range(3):
    out = solver.minimize(model, batch)
torch.cuda.synchronize()
assert np.isfinite(float(out["total_loss"]))
assert torch.cuda.current_device() == int(os.environ.get("LOCAL_RANK", "0"))
if os.environ.get("BD_TEST_HOST_BATCH") == "1":
    assert model._h2d.stager.device.index == torch.cuda.current_device() and model._h2d.dst.device.index == torch.cuda.current_device()
w = model.arena.w.cpu().numpy()
np.save(out_path, np.stack([w0.cpu().numpy(), w]))
sys.stderr.write("DIGEST " + hashlib.sha256(w.tobytes()).hexdigest() + " " + repr(float(np.abs(w).sum())) + "\n")
sys.stderr.flush()
if bdcomm.get_comm() is not None:
    bdcomm.get_comm().barrier()
os._exit(0)
"""


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run(tmp, tag, world=1, force=False, batch=4, model="retinanet", wire="", host_batch=False):
    port = _free_port()
    procs, outs = [], []
    for r in range(world):
        env = dict(os.environ, BD_FORCE_ALLREDUCE="1" if force else "0", HSA_ENABLE_IPC_MODE_LEGACY="0", BD_TEST_BATCH=str(batch),
                   BD_TEST_MODEL=model, BD_TEST_WIRE=wire, BD_TEST_HOST_BATCH="1" if host_batch else "0",
                   RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.pop("TORCHELASTIC_USE_AGENT_STORE", None)
        out = os.path.join(tmp, f"{tag}_{r}.npy")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, "-c", _SCRIPT, ROOT, out], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    digests = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=600)
            assert p.returncode == 0, se[-3000:]
            line = [l for l in se.splitlines() if l.startswith("DIGEST ")]
            assert line, se[-2000:]
            digests.append(line[-1].split()[1:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return digests, [np.load(o) for o in outs]


def test_rccl_bucket_path_is_bit_identical_to_the_local_step(tmp_path):
    plain, _ = _run(str(tmp_path), "plain")
    again, _ = _run(str(tmp_path), "again")
    assert plain == again, "the step itself is not reproducible"
    forced, _ = _run(str(tmp_path), "forced", force=True)
    assert forced == plain, (forced, plain)


def test_bf16_wire_buckets_stay_within_bf16_resolution(tmp_path):
    """SOLVER.ALLREDUCE_DTYPE = "bf16" (opt-in; bd_comm_allreduce_async_bf16): the buckets are rounded to bf16, all-reduced by RCCL as
    ncclBfloat16 and widened back on the communication stream.  With one rank the result is the rounded gradient: three steps end within
    bf16 resolution of the fp32 run (rel-L2 of the parameter change <= 1e-2: three steps of compounding 2^-9 roundings), and NOT equal to it."""
    _, plain = _run(str(tmp_path), "wplain")
    _, wire = _run(str(tmp_path), "wbf16", force=True, wire="bf16")
    assert np.array_equal(plain[0][0], wire[0][0])
    s0, s1 = plain[0][1] - plain[0][0], wire[0][1] - wire[0][0]
    rel = np.linalg.norm(s1 - s0) / np.linalg.norm(s0)
    assert 0 < rel < 1e-2, rel


def test_fcos_stats_allreduce_on_the_rccl_path_is_bit_identical_to_the_local_step(tmp_path):
    """FCOS adds the forward-side two-scalar all-reduce (ncclAvg of num_fg / sum ctr, models/det/fcos.py:143-144) on the solver's
    high-priority stream, interleaved with the bucket all-reduces on the communication stream of the SAME communicator."""
    plain, _ = _run(str(tmp_path), "fplain", model="fcos")
    forced, _ = _run(str(tmp_path), "fforced", force=True, model="fcos")
    assert forced == plain, (forced, plain)


def _device_count():
    import torch
    return torch.cuda.device_count()


def test_two_ranks_match_one_rank_on_the_concatenated_batch(tmp_path):
    if _device_count() < 2:
        pytest.skip("needs two GPUs (one process per GPU; RCCL refuses two ranks on one device)")
    d2, w2 = _run(str(tmp_path), "w2", world=2, batch=4)
    assert d2[0] == d2[1], "the two ranks ended with different parameters"
    assert np.array_equal(w2[0][0], w2[1][0]), "broadcast_parameters did not make rank 1 start from rank 0's parameters"
    _, w1 = _run(str(tmp_path), "w1", world=1, batch=4)
    assert np.array_equal(w1[0][0], w2[0][0])
    step2, step1 = w2[0][1] - w2[0][0], w1[0][1] - w1[0][0]
    rel = np.linalg.norm(step2 - step1) / np.linalg.norm(step1)
    # same mathematical update; the weight-gradient sums over pixels are split differently (2 + 2 images vs 4) and after the first
    # step the bf16 re-packed weights may round differently in their last bit
    assert rel < 2e-2, rel


def test_two_ranks_fcos_with_different_num_fg_match_one_rank(tmp_path):
    """The FCOS step with world 2: the ranks hold different numbers of foreground points; after the two-scalar mean all-reduce the
    averaged gradient equals the one-rank gradient on the concatenated batch."""
    if _device_count() < 2:
        pytest.skip("needs two GPUs (one process per GPU; RCCL refuses two ranks on one device)")
    d2, w2 = _run(str(tmp_path), "f2", world=2, batch=4, model="fcos")
    assert d2[0] == d2[1], "the two ranks ended with different parameters"
    _, w1 = _run(str(tmp_path), "f1", world=1, batch=4, model="fcos")
    assert np.array_equal(w1[0][0], w2[0][0])
    step2, step1 = w2[0][1] - w2[0][0], w1[0][1] - w1[0][0]
    rel = np.linalg.norm(step2 - step1) / np.linalg.norm(step1)
    assert rel < 2e-2, rel


def test_host_numpy_batch_takes_the_same_step_as_a_device_batch(tmp_path):
    """float64 host images through bd_h2d_submit (data_to_input's `Tensor(image)`): bit-identical parameters to the device-batch run --
    the float64 -> float32 conversion is the same rounding on both paths -- and the current device is untouched."""
    dev, _ = _run(str(tmp_path), "hdev")
    host, _ = _run(str(tmp_path), "hhost", host_batch=True)
    assert host == dev, (host, dev)


def test_two_ranks_with_host_numpy_batches(tmp_path):
    """Round-3 ADVICE (high): with `torch.device("cuda")` every rank passed device 0 to bd_h2d_create and the staging threads of rank 1
    copied into device 0.  Two ranks fed host batches must end with the parameters of the two-rank device-batch run."""
    if _device_count() < 2:
        pytest.skip("needs two GPUs (one process per GPU; RCCL refuses two ranks on one device)")
    d_dev, _ = _run(str(tmp_path), "h2dev", world=2, batch=4)
    d_host, _ = _run(str(tmp_path), "h2host", world=2, batch=4, host_batch=True)
    assert d_host[0] == d_host[1] and d_host == d_dev, (d_host, d_dev)
