"""Inputs of the one-epoch sizing tests (test code only): optimiser states, forces, beams and the early-stop state of
every case, all seeded.  The CPU test of the references (tests/test_sizing_step_reference.py) and the GPU test of the
kernels (tests/test_gpu_sizing_step.py) draw the same inputs, so the error bounds measured on the CPU hold for what the
GPU runs."""
import functools
import types

import numpy as np

from oracle import beam_oracle as bo
from oracle import sizing_oracle as so

EPS32 = 2.0 ** -23
T_STEPS = (0, 1, 17)                 # plus max_epochs - 1, which the cases of kind "d" take
KINDS = "aecdb"                      # case b of a batch is of kind KINDS[(b + shift) % 5]:
#   a  improving                      best = loss, cnt = 0                 continues
#   b  not improving, cnt + 1 < patience   cnt + 1                         continues
#   c  not improving, cnt + 1 == patience                                  stops
#   d  improving, t + 1 == max_epochs                                      stops
#   e  active = 0                                                          untouched
CLAMP_I, CLAMP_M, CLAMP_V = 5e-3, 1.0, 1e-4      # an element whose Adam step lands below clamp_min (while its forces are ~0)


def beam_hp():
    """The beam script's hyper-parameters, as `SizingConfig().c_params()` passes them."""
    from openpystruct_amd import sizing
    return sizing.SizingConfig().c_params()


def frame_hp():
    """What openpystruct_amd/frames.py passes: no scheduler (gamma = 1), bend_eps = 1e-8, the frame script's constants."""
    from openpystruct_amd import _cabi, frames
    cfg = frames.FrameConfig()
    return _cabi.SizingParams(E=cfg.E, G=cfg.G, alpha_moment=cfg.alpha_moment, alpha_shear=cfg.alpha_shear, lr=cfg.lr, gamma=1.0,
                              beta1=0.9, beta2=0.999, adam_eps=1e-8, clamp_min=1e-8, bend_eps=1e-8, area_coef=cfg.k,
                              tolerance=cfg.tolerance, patience=cfg.patience, max_epochs=cfg.num_epochs)


def clamp_columns(Ne):
    """The elements of every row that are clamp elements: the last min(2, Ne // 2) (none when the row has one element)."""
    return np.arange(Ne - min(2, Ne // 2), Ne)


def optimiser_state(rng, B, Ne):
    """I log-uniform in [3e-3, 0.75], exp_avg ~ N(0, 1), exp_avg_sq = U(0.5, 2) exp_avg^2 (float32), clamp elements set."""
    I = np.exp(rng.uniform(np.log(3e-3), np.log(0.75), size=(B, Ne))).astype(np.float32)
    m = rng.standard_normal((B, Ne)).astype(np.float32)
    v = (rng.uniform(0.5, 2.0, size=(B, Ne)) * m.astype(np.float64) ** 2).astype(np.float32)
    c = clamp_columns(Ne)
    I[:, c], m[:, c], v[:, c] = CLAMP_I, CLAMP_M, CLAMP_V
    return I, m, v


def random_forces(rng, B, Ne):
    """Shear ~ 1e5 N(0, 1), moment ~ 2e6 N(0, 1) (float64); zero on the clamp elements."""
    V, M = 1e5 * rng.standard_normal((B, Ne)), 2e6 * rng.standard_normal((B, Ne))
    c = clamp_columns(Ne)
    V[:, c], M[:, c] = 0.0, 0.0
    return V, M


def beams(rng, B, Ne, per_case):
    """Straight beams on a non-uniform mesh: node 1 and 1 to 3 interior rollers fixed in u_y, 1 to 4 point loads of 1e4 .. 1e6 of
    either sign on the nodes between them, a line load.  The rollers sit at jittered even spacings, the last one three elements
    before the free end (so the clamp elements at the end carry the line load only), and long meshes take at least 2 (Ne > 48) or 3
    (Ne > 100) of them: no span exceeds ~50 elements, which keeps the Jacobi-scaled condition number below 2^-24 / eps64 (checked
    by the tests) -- the float64 solves of kernel and reference then agree to half a float32 ulp of a row's largest force.
    per_case: x, fix [B, N], E, wy [B, Ne] differ from case to case; else one x, fix [N] and scalar E, wy.  Fy [B, N] always."""
    N, G = Ne + 1, (B if per_case else 1)
    x = np.concatenate([np.zeros((G, 1)), np.cumsum(rng.uniform(0.3, 0.7, size=(G, Ne)), axis=1)], axis=1)
    fix = np.zeros((G, N), dtype=np.uint8)
    fix[:, 0] = 1
    last = max(N - 4, 1)                          # Ne = 1: the second support is the end node
    for g in range(G):
        nr = min(int(rng.integers(1 + (Ne > 48) + (Ne > 100), 4)), last)
        pos = np.round(last * (np.arange(1, nr + 1) + rng.uniform(-0.1, 0.1, size=nr)) / nr).astype(np.int64)
        pos[-1] = last
        fix[g, np.clip(pos, 1, last)] = 1
    Fy = np.zeros((B, N))
    for b in range(B):
        free = np.flatnonzero(fix[b if per_case else 0, :last + 1] == 0)
        if free.size:
            nodes = rng.choice(free, size=min(int(rng.integers(1, 5)), free.size), replace=False)
            Fy[b, nodes] = rng.choice([-1.0, 1.0], size=nodes.size) * np.exp(rng.uniform(np.log(1e4), np.log(1e6), size=nodes.size))
    if per_case:
        E, wy = 200e9 * rng.uniform(0.8, 1.2, size=(B, Ne)), rng.uniform(-1500.0, -500.0, size=(B, Ne))
        return x, fix, E, wy, Fy
    return x[0], fix[0], np.float64(200e9), np.float64(-1000.0), Fy


def beam_forces(x, E, I32, fix, Fy, wy):
    """V, M [B, Ne] of the float64 dense solve, one beam at a time, on the float32 inertias widened to double; its status [B]."""
    I = np.asarray(I32, dtype=np.float32).astype(np.float64)
    _, _, V, M, st = bo.solve_beam_batched(x, E, I, fix, Fy, wy)
    return V, M, st


def case_states(ref_loss, hp, shift, group):
    """Early-stop state of every case before the call, chosen from the reference's loss so that each stop decision is 2e-3
    (relative) away from its threshold `best - tolerance`: kinds as KINDS, t, best (float32), cnt, active.  Batches of at least
    2 * group + 1 cases hold one whole group (wavefront) of inactive cases, cases group .. 2 * group - 1."""
    B = ref_loss.shape[0]
    kind = np.array([KINDS[(b + shift) % 5] for b in range(B)])
    if group > 1 and B >= 2 * group + 1:
        kind[group:2 * group] = "e"
    t = np.array([T_STEPS[(b + shift) % 3] for b in range(B)], dtype=np.int32)
    t[kind == "d"] = hp.max_epochs - 1
    thr = ref_loss + hp.tolerance                               # loss < best - tolerance  <=>  best > thr
    improving = (kind == "a") | (kind == "d")
    best = np.where(improving, thr * (1 + 2e-3), thr * (1 - 2e-3))
    best[(kind == "a") & (np.arange(B) % 2 == 1)] = np.inf      # the first epoch's state
    cnt = np.select([kind == "b", kind == "c"], [hp.patience - 2, hp.patience - 1], default=1).astype(np.int32)
    assert hp.patience >= 2
    return types.SimpleNamespace(kind=kind, t=t, best=best.astype(np.float32), cnt=cnt, active=(kind != "e").astype(np.uint8))


def reference_epoch(I, m, v, V, M, hp, shift, group):
    """States of the batch's cases and the float64 reference of the epoch they are about to run.  The loss does not depend on
    t, best or cnt, so one evaluation places `best`, a second one decides."""
    B = I.shape[0]
    z = np.zeros(B, dtype=np.int64)
    loss = so.sizing_step_reference(I, m, v, V, M, z, np.full(B, np.inf), z, hp)["loss"]
    st = case_states(loss, hp, shift, group)
    ref = so.sizing_step_reference(I, m, v, V, M, st.t, st.best, st.cnt, hp)
    # every decision sits where case_states put it, far from float32 round-off
    assert (np.abs(st.best.astype(np.float64) - hp.tolerance - ref["loss"]) >= 1e-3 * np.abs(ref["loss"] + hp.tolerance))[st.kind != "e"].all()
    want_stop = (st.kind == "c") | (st.kind == "d")
    assert (ref["stop"][st.kind != "e"] == want_stop[st.kind != "e"]).all()
    return st, ref


@functools.lru_cache(maxsize=None)
def fused_case(Ne, B, per_case, seed=0):
    """Beams, optimiser state and reference forces of one fused-epoch batch (cached: several tilings run the same batch)."""
    rng = np.random.default_rng([Ne, B, int(per_case), seed])
    x, fix, E, wy, Fy = beams(rng, B, Ne, per_case)
    I, m, v = optimiser_state(rng, B, Ne)
    V, M, st = beam_forces(x, E, I, fix, Fy, wy)
    assert (st == 0).all()
    return types.SimpleNamespace(x=x, fix=fix, E=E, wy=wy, Fy=Fy, I=I, m=m, v=v, V=V, M=M)


def fused_kappa(Ne, B, per_case):
    """The largest Jacobi-scaled condition number among the beams of fused_case(Ne, B, per_case)."""
    from tests import helpers
    c = fused_case(Ne, B, per_case)
    return max(helpers.kappa_scaled(c.x[b] if per_case else c.x, c.E[b] if per_case else float(c.E), c.I[b].astype(np.float64),
                                    c.fix[b] if per_case else c.fix) for b in range(B))


# Error bounds of tests/test_gpu_sizing_step.py in eps32, for all four quantities of sizing_step_errors.
STEP_BOUND = 16.0        # stand-alone kernels: float32 round-off alone reaches 6.9 (tests/test_sizing_step_reference.py)
FUSED_BOUND = 36.5       # fused epoch: 4 x 9.11, the float32 step on forces moved by one float32 ulp (same file)

TILING_ROWS = 0x200      # OPS_AMD_TILING_ROWS
# The fused-epoch batches: (tiling, per-case geometry, lanes per beam P and elements per lane M of the kernel that serves it,
# (Ne, B) shapes).  64 / P cases share a wavefront.  Every kernel meets odd and even Ne, a full last wave and -- while a wave
# holds more than one case -- a ragged one, and a wave whose cases are all inactive (B >= 2 * 64 / P + 1).  Tiling 0 picks the
# row-staged 16-lane kernel for shared geometry up to Ne = 111, then the first classic tiling that fits: <32, 4>, <64, 4>.
FUSED_TABLE = (
    (0, False, 16, 7, ((1, 1), (1, 4), (2, 3), (2, 9), (5, 5), (5, 9), (99, 3), (99, 9), (100, 4), (100, 5), (111, 1), (111, 9))),
    (16, False, 16, 7, ((5, 4), (5, 9), (99, 3), (99, 4), (100, 3), (100, 9), (111, 4), (111, 9))),
    (16, True, 16, 7, ((5, 4), (5, 9), (99, 3), (99, 4), (100, 3), (100, 9), (111, 4), (111, 9))),
    (0, True, 16, 7, ((99, 9), (100, 3))),
    (8, False, 8, 13, ((7, 8), (7, 17), (102, 7), (102, 17), (103, 8), (103, 17))),
    (8, True, 8, 13, ((7, 17), (102, 8), (103, 7), (103, 17))),
    (32, False, 32, 4, ((64, 1), (64, 2), (126, 3), (127, 2), (127, 3), (127, 5))),
    (32, True, 32, 4, ((64, 3), (126, 2), (127, 5))),
    (64, False, 64, 2, ((112, 1), (112, 2), (127, 1), (127, 2))),
    (64, True, 64, 2, ((112, 2), (127, 2))),
    (0, False, 32, 4, ((112, 1), (112, 2), (127, 1), (127, 2))),
    (64, False, 64, 4, ((128, 1), (128, 2))),
    (64, True, 64, 4, ((128, 2),)),
    (0, False, 64, 4, ((128, 1), (128, 2))),
)
