"""Golden fixtures for the trainer at the two board sizes whose 128-filter network the other fixtures do not cover:
19x19 (config C5's board) and 6x6 (the reference's default BOARD_SIZE), from the REFERENCE's own
loss.py:calculate_loss in float32 on the CPU (the output is committed; the reference is read at run time only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trainer_sizes.py <reference checkout> c19full
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trainer_sizes.py <reference checkout> c6w128full

train_loss_c19full.npz / train_loss_c6w128full.npz: 128 filters, 2 blocks, a batch of 16 games live for all 5 unroll
steps (the well-conditioned batch of train_loss_c128full.npz, see make_golden_trainer.py, whose format — batch, IS
weights, H / blocks / filters, augmentation draw, loss, components, td errors, gradient norms and the small gradients —
and per-name seeded weight stream these files share, so tests/test_trainer.py reads them as it reads that one)."""
import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF, VARIANT = sys.argv[1], sys.argv[2]
H = {"c19full": 19, "c6w128full": 6}[VARIANT]
BLOCKS, FILTERS = 2, 128
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
for name in ("seaborn",):
    sys.modules.setdefault(name, types.ModuleType(name))
_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules.setdefault("torch.utils.tensorboard", _tb)
os.chdir(tempfile.mkdtemp(prefix="gmz_golden_tr_"))

import torch  # noqa: E402

import config as ref_config_mod  # noqa: E402
cfg = ref_config_mod.config
cfg.BOARD_SIZE, cfg.ACTION_SPACE_SIZE, cfg.NUM_RES_BLOCKS, cfg.NUM_FILTERS = H, H * H, BLOCKS, FILTERS
import network as ref_net  # noqa: E402
import loss as ref_loss  # noqa: E402

torch.set_num_threads(1)


def synth_weights(shapes, base):
    """make_golden_trainer.py's per-name seeded stream (tests/test_trainer.py regenerates it)."""
    out = {}
    for name, shape in shapes.items():
        r = np.random.RandomState((zlib.crc32(name.encode()) ^ base) & 0x7FFFFFFF)
        if name.endswith("num_batches_tracked"):
            out[name] = np.zeros(shape, np.int64)
        elif "running_var" in name:
            out[name] = (0.5 + r.rand(*shape)).astype(np.float32)
        elif "running_mean" in name:
            out[name] = (0.1 * r.randn(*shape)).astype(np.float32)
        elif ("bn" in name) and name.endswith("weight"):
            out[name] = (0.5 + 0.5 * r.rand(*shape)).astype(np.float32)
        elif name.endswith("bias"):
            out[name] = (0.05 * r.randn(*shape)).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            out[name] = (r.randn(*shape) / np.sqrt(fan_in)).astype(np.float32)
    return out


def seeded(base):
    m = ref_net.GomokuNetEZ(cfg)
    sd = synth_weights({k: tuple(v.shape) for k, v in m.state_dict().items()}, base)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


B, U, A = 16, cfg.NUM_UNROLL_STEPS, H * H
rs = np.random.RandomState(5)
obs = (rs.rand(B, U + 1, 3, H, H) < 0.3).astype(np.float32)
act = rs.randint(0, A, (B, U)).astype(np.int64)  # every game live for all unroll steps
rew = rs.choice([-1.0, 0.0, 1.0], (B, U)).astype(np.float32)
pol = rs.dirichlet(np.ones(A), (B, U + 1)).astype(np.float32)
val = rs.uniform(-1, 1, (B, U + 1)).astype(np.float32)
isw = rs.uniform(0.2, 1.0, B).astype(np.float32)
batch = [torch.from_numpy(x) for x in (obs, act, rew, pol, val)]
out = dict(obs=obs, act=act, rew=rew, pol=pol, val=val, isw=isw, H=H, blocks=BLOCKS, filters=FILTERS)
want, seed = (1, True), 0  # the np seed whose (k, flip) draw is the other 128-filter fixtures' augmentation
while True:
    np.random.seed(seed)
    if (np.random.randint(4), bool(np.random.choice([True, False]))) == want:
        break
    seed += 1
model, target = seeded(10), seeded(20)
np.random.seed(seed)
loss, logs = ref_loss.calculate_loss(model, target, batch, torch.from_numpy(isw))
loss.backward()
out.update({"c0/k": want[0], "c0/flip": want[1], "c0/loss": np.float64(logs[0]),
            "c0/comps": np.array(logs[1:5], np.float64), "c0/td": np.asarray(logs[5], np.float32)})
for k, p in model.named_parameters():  # gradients: every norm, full values of the small tensors
    g = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    out["c0/gn/" + k] = np.float64(np.linalg.norm(g.astype(np.float64)))
    if g.size <= 4096:
        out["c0/g/" + k] = g
print("%s: k %d flip %s loss %.6f comps %s" % (VARIANT, want[0], want[1], logs[0], np.array(logs[1:5])))
np.savez_compressed(os.path.join(HERE, "train_loss_%s.npz" % VARIANT), **out)
