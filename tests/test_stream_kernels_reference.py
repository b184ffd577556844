"""tests/stream_kernels_ref.py on the CPU: (1) the float64 references against float64 torch autograd of the plain composition at every
table case -- F.conv1d + F.batch_norm, sum -> F.batch_norm -> leaky_relu -> the mirrored mask, CompositeLoss / TrainableL1L2Loss,
clip_grad_norm_ + torch.optim.Adam / AdamW -- so no hand-written derivative stands unchecked; (2) the float32 evaluation of every
documented formula through the very protocol tests/test_gpu_stream_kernels.py runs, whose largest constants are
stream_kernels_ref.CPU_CONST (the GPU bounds are four times these); (3) teeth: every wrong variant in BUGS violates the GPU bound or
an exact condition on the outputs it should break; (4) the streams: the mask mirror has no ties but the one planted, every dropout
case keeps and drops in every column, the noise mirror is ip_mix, and Adam's 1 - beta convention is stated.
"""
import functools

import numpy as np
import pytest

from tests import stream_kernels_ref as R

torch = pytest.importorskip("torch")
F = torch.nn.functional
f32, f64 = np.float32, np.float64
_ids = lambda v: v if isinstance(v, str) else "-".join(map(str, v))      # noqa: E731


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=f64), dtype=torch.float64, requires_grad=grad)


def _agree(name, ref_unit, want):
    ref, unit = ref_unit
    want = want.detach().numpy().reshape(np.shape(ref))
    assert (np.abs(ref - want) <= 1e-12 * np.maximum(unit, np.abs(ref))).all(), (name, float(np.abs(ref - want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# (1) the references against autograd
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SB_CASES, ids=_ids)
def test_stencil_bn_reference_against_autograd(case):
    B, Fe, _ = case
    i = R.sb_inputs(case)
    y0 = F.conv1d(_t(i["x"]).unsqueeze(1), _t(i["cw"]).view(1, 1, 3), _t(i["cb"]), padding=1)
    if case[2]:                                          # the input is built so that |mean(y)| / std(y) is the case's ratio
        assert abs(abs(float(y0.mean())) / float(y0.std(unbiased=False)) - case[2]) < 1e-3 * case[2]
    for tr in (1, 0):
        x, cw, cb, gamma, beta = (_t(i[k], True) for k in ("x", "cw", "cb", "gamma", "beta"))
        rm, rv = _t(i["rmean"]), _t(i["rvar"])
        ref = R.stencil_bn_fwd(i["x"], i["cw"], i["cb"], i["gamma"], i["beta"], R.SB_EPS, R.SB_MOM, tr, i["rmean"], i["rvar"], 2)
        eps, mom = float(f32(R.SB_EPS)), float(f32(R.SB_MOM))
        for _ in range(2):
            y = F.conv1d(x.unsqueeze(1), cw.view(1, 1, 3), cb, padding=1)
            if B * Fe == 1 and tr:                       # one value: F.batch_norm refuses; mean = y, var = 0
                z = (y - y.detach()) * gamma / np.sqrt(eps) + beta
                rm, rv = (1 - mom) * rm + mom * y.detach().reshape(1), (1 - mom) * rv
            else:
                z = F.batch_norm(y, rm, rv, gamma, beta, bool(tr), mom, eps)
        _agree("z", ref["z32"], z)
        _agree("rmean", ref["rmean"], rm)
        _agree("rvar", ref["rvar"], rv)
        if tr and B * Fe > 1:
            _agree("mean", ref["mean"], y.mean())
            _agree("invstd", ref["invstd"], 1 / torch.sqrt(y.var(unbiased=False) + eps))
        # the backward on the exact float64 forward
        save = np.array([ref["mean"][0], ref["invstd"][0]])
        bwd = R.stencil_bn_bwd(i["x"], i["g32"], False, i["cw"], i["cb"], i["gamma"], save, tr)
        z.backward(_t(i["g32"]).view_as(z))
        _agree("dx", bwd["dx"], x.grad)
        for k, name in enumerate(("dw0", "dw1", "dw2")):
            _agree(name, bwd[name], cw.grad[k])
        _agree("db", bwd["db"], cb.grad)
        _agree("dgamma", bwd["dgamma"], gamma.grad)
        _agree("dbeta", bwd["dbeta"], beta.grad)


@pytest.mark.parametrize("case", R.FB_CASES, ids=_ids)
def test_fused_bn_reference_against_autograd(case):
    B, Fe, na, bf, norm, slope, p, training, running, zs = case
    i = R.fb_inputs_cached(case)
    keep = R.fb_keep(case)
    xs = [_t(R._wide(a, bf, f64), True) for a in i["xs"]]
    z = xs[0]
    for a in xs[1:]:
        z = z + a
    zref, _ = R.fb_sum(i["xs"], bf)
    _agree("sum", (zref, np.abs(zref)), z)
    if bf and na > 1:
        return _fused_bn_from_stored(case, i, keep)       # the rounded sum is not differentiable: from the stored z on
    _fused_bn_from_stored(case, i, keep, z, xs)


def _fused_bn_from_stored(case, i, keep, z=None, xs=None):
    B, Fe, na, bf, norm, slope, p, training, running, zs = case
    zst = R.fb_stored_sum(i["xs"], bf)
    gm, be = (i["gamma"], i["beta"]) if norm else (None, None)
    leaf = _t(zst, True)
    zz = leaf if z is None or (na > 1) else z             # float32 sums differ from the exact sum: differentiate at the stored z
    ref = R.fused_bn_fwd(zst, bf, gm, be, R.FB_EPS, R.FB_MOM, training, i["rmean"], i["rvar"], slope, p, keep)
    gamma, beta = (_t(gm, True), _t(be, True)) if norm else (None, None)
    rm, rv = _t(i["rmean"]), _t(i["rvar"])
    eps, mom = float(f32(R.FB_EPS)), float(f32(R.FB_MOM))
    y = F.batch_norm(zz, rm, rv, gamma, beta, bool(training), mom, eps) if norm else zz
    if norm and training:
        _agree("mean", ref["mean"], zz.mean(0))
        _agree("rstd", ref["rstd"], 1 / torch.sqrt(zz.var(0, unbiased=False) + eps))
        _agree("rmean", ref["rmean"], rm)
        _agree("rvar", ref["rvar"], rv)
    if slope is not None:
        y = F.leaky_relu(y, float(f32(slope)))
    mult = _t(keep / (1.0 - float(f32(p)))) if training and p > 0 else _t(np.ones((B, Fe)))
    y = y * mult
    _agree("y", ref["y"], y)
    if not training:
        return
    # the backward on the exact float64 statistics
    if norm:
        mean, rstd = ref["mean"][0], ref["rstd"][0]
    else:
        mean = rstd = None
    bwd = R.fused_bn_bwd(i["dy"], bf, zst, mean, rstd, gm, be, slope, p, keep)
    y.backward(_t(R._wide(i["dy"], bf, f64)))
    _agree("dz", bwd["dz"], leaf.grad if zz is leaf else xs[0].grad)
    if norm:
        _agree("dgamma", bwd["dgamma"], gamma.grad)
        _agree("dbeta", bwd["dbeta"], beta.grad)


@pytest.mark.parametrize("case", R.FL_CASES, ids=_ids)
def test_loss_reference_against_the_modules(case):
    from openpystruct_amd.surrogates import CompositeLoss, TrainableL1L2Loss
    B, C, nI, nD, box, alpha, alpha0, bf = case
    nR = C - nI - nD
    i = R.fl_inputs(case)
    lo, hi = R.fl_box(case)
    ref = R.surrogate_loss_grad(i["p"], bf, i["t"], nI, nD, alpha, alpha0, lo, hi, R.FL_BOX_W, R.FL_PENALTY, R.FL_SUM0, 2)
    p, t = _t(R._wide(i["p"], bf, f64), True), _t(i["t"])
    kw = dict(min_constraint=None if lo is None else float(f32(lo)), max_constraint=None if hi is None else float(f32(hi)))
    w, pen, a32 = float(f32(R.FL_BOX_W)), float(f32(R.FL_PENALTY)), float(f32(alpha))
    if nD > 0 and nR > 0:
        crit = CompositeLoss(nI, nD, nR, a32, w, penalty_pinn=pen, **kw).double()
        crit.l1l2_loss.alpha.data.fill_(a32)
        loss = crit(p, t)
    else:                                                # an empty group has no mean: the module's terms for the groups there are
        crit = TrainableL1L2Loss(a32, penalty_weight=w, **kw).double()
        crit.alpha.data.fill_(a32)
        loss = crit(p[:, :nI], t[:, :nI])
        if C > nI:
            loss = loss + pen * torch.mean(torch.abs(p[:, nI:] - t[:, nI:]) / (torch.abs(t[:, nI:]) + 1e-8))
    if alpha0 == alpha0:
        loss = loss + (float(f32(alpha0)) - a32) ** 2
    loss.backward()
    _agree("loss", (ref["loss"][0], ref["loss"][1]), loss)
    _agree("grad", ref["grad"], p.grad)
    once = float(f32(ref["loss"][0]))
    assert abs(float(ref["loss_sum"][0]) - (float(f32(R.FL_SUM0)) + 2 * once)) <= 1e-12 * float(ref["loss_sum"][1])
    # what the case plants is there: p == t (an exact zero of the gradient unless a box term acts), p on a bound, t == 0
    pv, tv = R._wide(i["p"], bf, f64), i["t"].astype(f64)
    assert (pv == tv).any()
    if B * nI >= 3:
        assert (pv[:, :nI] == R.FL_LO).any() and (pv[:, :nI] == R.FL_HI).any()
    if B * max(nD, nR) >= 2:                             # a group of one element holds p == t alone
        assert (tv[:, nI:] == 0).any()
        assert (ref["grad"][1][:, nI:] > 1e7 * R.FL_PENALTY / (B * max(nD, nR))).any()      # the unit carries the 1e8 factor


@pytest.mark.parametrize("case", [c for c in R.FA_CASES if c[0] <= 131072 + 7], ids=_ids)
def test_adam_reference_against_torch_optim(case):
    """clip_grad_norm_ + torch.optim.Adam / AdamW in float64 with the float32-rounded hyper-parameters (1 - beta is then exact in
    float64, the kernel's contract), two steps with lr changed in between."""
    n, cfg = case[0], R.fa_config(case)
    i = R.fa_inputs(case)
    h = lambda v: float(f32(v))      # noqa: E731
    par = torch.nn.Parameter(_t(i["p"]))
    cls = torch.optim.AdamW if cfg["flags"] & R.DECOUPLED else torch.optim.Adam
    opt = cls([par], lr=h(R.FA_LRS[0]), betas=(h(R.FA_B1), h(R.FA_B2)), eps=h(R.FA_EPS), weight_decay=h(cfg["wd"]), foreach=False, fused=False)
    opt.state[par] = dict(step=torch.tensor(float(cfg["step0"])), exp_avg=_t(i["m"]), exp_avg_sq=_t(i["v"]))
    state = dict(p=i["p"].astype(f64), m=i["m"].astype(f64), v=i["v"].astype(f64))
    for k in range(2):
        g = i["g"] if k == 0 else R.fa_second_gradient(case, i["g"])
        normsq = R.fa_partials(g, cfg["grad_scale"], cfg["parts"]).sum() if cfg["parts"] else None
        ref = R.flat_clip_adam_step(state["p"], g, state["m"], state["v"], R.FA_LRS[k], cfg["step0"] + k + 1,
                                    cfg["max_norm"], cfg["grad_scale"], R.FA_B1, R.FA_B2, R.FA_EPS, cfg["wd"], cfg["flags"], normsq)
        par.grad = _t(g) * h(cfg["grad_scale"])
        if cfg["max_norm"] > 0:
            torch.nn.utils.clip_grad_norm_([par], h(cfg["max_norm"]))
        opt.param_groups[0]["lr"] = h(R.FA_LRS[k])
        opt.step()
        st = opt.state[par]
        _agree("p", ref["p"], par.data)
        _agree("m", ref["m"], st["exp_avg"])
        _agree("v", ref["v"], st["exp_avg_sq"])
        state = {name: ref[name][0] for name in ("p", "m", "v")}


# ---------------------------------------------------------------------------------------------------------------------------------
# (2) the float32 evaluation: the constants behind the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_CASES = [(kind, case) for kind, (_, cases) in R.PROTOCOLS.items() for case in cases]


@functools.lru_cache(maxsize=None)
def case_constants(kind, case, bug=()):
    return R.measure(R.PROTOCOLS[kind][0](case, R.CpuImpl(bug)))


@pytest.mark.parametrize("kind,case", ALL_CASES, ids=_ids)
def test_float32_evaluation_stays_inside_the_table(kind, case):
    ratios, absr, failed = case_constants(kind, case)
    print(kind, case, "  ".join(f"{k} {v:.2f}" for k, v in {**ratios, **absr}.items()))
    assert not failed, failed
    for name, v in ratios.items():
        assert v <= R.CPU_CONST[name], (name, v)
    for name, v in absr.items():                          # the mirror against itself: only the rounding of the stored value
        assert v <= 1.0, (name, v)


def test_table_of_constants_is_what_was_measured():
    """One line per output (pytest -s): the largest measured constant, the table's entry and the GPU bound.  An entry of the table is
    the measurement plus about 12 %, rounded up: a slack entry would be a slack bound, so none may exceed 1.5 x measured + 0.1."""
    measured = {name: 0.0 for name in R.CPU_CONST}
    for kind, case in ALL_CASES:
        for name, v in case_constants(kind, case)[0].items():
            measured[name] = max(measured[name], v)
    assert set(measured) == set(R.CPU_CONST)
    assert R.SIDE_MARGIN >= max(R.bound_constant("fb.y"), R.bound_constant("fb.dz"))
    for name in R.CPU_CONST:
        print(f"{name:12s} measured {measured[name]:6.2f}   table {R.CPU_CONST[name]:5.2f}   GPU bound {R.bound_constant(name):6.2f}")
    for name in R.CPU_CONST:
        if name in R.BF16_TWINS:                         # held to its float32 twin's constant
            assert measured[name] <= R.CPU_CONST[name]
        else:
            assert measured[name] <= R.CPU_CONST[name] <= 1.5 * measured[name] + 0.1, name


# ---------------------------------------------------------------------------------------------------------------------------------
# (3) teeth
# ---------------------------------------------------------------------------------------------------------------------------------
BUGS = [("taps_reversed", "sb", ("sb.z32", "sb.z16", "sb.dx", "sb.dw0", "sb.dw2")),              # w0 <-> w2
        ("pad_from_neighbour_row", "sb", ("sb.z32", "sb.dx", "sb.dw0", "sb.dw2")),               # x[r][-1] read as x[r - 1][F - 1]
        ("biased_running_var", "sb", ("sb.rvar",)),
        ("momentum_on_old", "sb", ("sb.rmean", "sb.rvar")),                                      # (1 - momentum) on the new value
        ("frozen_as_training", "sb", ("sb.dx", "sb.db")),                                        # mean(g), mean(g yhat) subtracted in eval
        ("mask_transposed", "fb", ("fb.y", "mask is the mirror's at r F + c")),                  # c B + r
        ("keep_gt", "fb", ("fb.y", "mask is the mirror's at r F + c")),                          # keep when u > p
        ("no_ks_bwd", "fb", ("fb.dz", "fb.dgamma", "fb.dbeta")),                                 # 1 / (1 - p) left out of the backward
        ("side_from_z", "fb", ("fb.y", "fb.dz")),                                                # LeakyReLU side from z
        ("var_bm1", "fb", ("fb.rstd", "fb.y")),                                                  # variance / (B - 1)
        ("drop_second", "fb", ("fb.zsave",)),                                                    # second addend dropped
        ("no_bf16_round", "fb", ("fb.y", "fb.mean")),                                            # bf16 sum normalised unrounded
        ("swap_inv", "fl", ("fl.grad",)),                                                        # inv_nD <-> inv_nR
        ("no_clamp", "fl", ("fl.grad", "fl.loss")),
        ("box_ge", "fl", ("fl.grad",)),                                                          # >= at the box bounds
        ("sign0_is_1", "fl", ("fl.grad",)),
        ("sum_overwrite", "fl", ("fl.loss_sum",)),
        ("late_correction", "fa", ("fa.p",)),
        ("eps_in_sqrt", "fa", ("fa.p",)),
        ("l2_for_decoupled", "fa", ("fa.p", "fa.m", "fa.v")),
        ("clip_no_scale", "fa", ("fa.p", "fa.m", "fa.v")),
        ("tail_unchanged", "fa", ("fa.p", "fa.m", "fa.v")),
        ("shadow_truncated", "fa", ("fa.shadow", "shadow is the new parameter rounded to nearest even"))]


@pytest.mark.parametrize("bug,kind,outputs", BUGS, ids=[b for b, _, _ in BUGS])
def test_wrong_variants_violate_the_gpu_bound(bug, kind, outputs):
    broken = set()
    for case in R.PROTOCOLS[kind][1]:
        if kind == "fa" and case[0] > 1025:
            continue
        ratios, absr, failed = case_constants(kind, case, bug)
        broken |= {name for name, v in ratios.items() if v > R.bound_constant(name)} | set(failed)
    print(f"{bug}: caught on {sorted(broken)}")
    assert broken >= set(outputs), (bug, kind, sorted(broken))


@pytest.mark.parametrize("bug", ["call_not_plus_1", "row_index"])
def test_wrong_noise_mappings_move_almost_every_element(bug):
    """A wrong call or index mapping moves more than 99 % of the elements by more than 0.01 sigma (the bound is 0.002 sigma)."""
    for case in R.IP_CASES:
        B, Fe, off, bf, C, counter, sigma = case
        if not sigma or B * Fe < 1000 or (bug == "row_index" and B == 1):
            continue
        i = R.ip_inputs(case)
        call = 0 if counter is None else counter
        good = R.gather_rows_noise(i["X"], i["idx"], sigma, R.SEED, call)["out"][1]
        bad = R.gather_rows_noise(i["X"], i["idx"], sigma, R.SEED, call, (bug,))["out"][1]
        moved = np.abs(good - bad) > 0.01 * sigma
        if bug == "row_index":
            moved = moved[1:]                            # the first row's index is its own
        assert moved.mean() > 0.99, (bug, case, moved.mean())
        print(f"{bug}: caught, {100 * moved.mean():.2f} % of {case[:2]} moved")


# ---------------------------------------------------------------------------------------------------------------------------------
# (4) the streams, and Adam's 1 - beta
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mask_mirror_ties_and_columns():
    """u sits on the 2^-24 grid: against p = float32(0.1) (off that grid) no tie exists; against p = 0.5 the one tie of the table is the
    planted one, which u >= p keeps.  Every dropout case keeps and drops in every column."""
    assert float(f32(0.1)) * 2.0 ** 24 != round(float(f32(0.1)) * 2.0 ** 24)
    ties = 0
    for case in R.FB_CASES:
        B, Fe, p, training = case[0], case[1], case[6], case[7]
        if not (training and p > 0):
            continue
        seed, call = R.fb_seed_call(case)
        assert seed >> 62 == 1
        u = R.bs.drop_uniform(R.bs.drop_key(seed, call), np.arange(B * Fe, dtype=np.uint64)).reshape(B, Fe)
        keep = R.fb_keep(case)
        assert np.array_equal(keep, u >= float(f32(p)))
        assert keep.any(0).all() and (~keep).any(0).all(), case
        tie = u == float(f32(p))
        ties += int(tie.sum())
        if case == R.FB_TIE_CASE:
            assert tie.reshape(-1)[R.FB_TIE_INDEX] and tie.sum() == 1 and keep.reshape(-1)[R.FB_TIE_INDEX]
        else:
            assert not tie.any()
    assert ties == 1


def test_noise_mirror_is_ip_mix():
    """input_noise against a scalar transcription of input_noise.hpp in Python integers, and its first moments."""
    def scalar(seed, call, i):
        m = R.MASK64
        z = (seed + R.IP_GOLDEN * (call + 1) + i * R.IP_SALT) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        u1, u2 = ((z >> 40) + 1) / 2 ** 24, ((z >> 16) & 0xFFFFFF) / 2 ** 24
        return np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    for call in R.COUNTERS:
        idx = np.array([0, 1, 7, 683, 2 ** 31 + 5], dtype=np.uint64)
        got = R.input_noise(R.SEED, call, idx)
        assert np.array_equal(got, np.array([scalar(R.SEED, call, int(k)) for k in idx]))
    n = R.input_noise(R.SEED, 5, np.arange(200000, dtype=np.uint64))
    assert abs(n.mean()) < 0.01 and abs(n.std() - 1) < 0.01 and np.abs(n).max() <= np.sqrt(2 * 24 * np.log(2))


def test_adam_one_minus_beta_convention():
    """FlatClipAdam hands betas to `float` arguments: the kernel forms 1.0f - float32(beta) (exact), torch.optim.Adam float(1 - beta).
    The distance between the two conventions, relative: on the moment's increment at most 2^-24 / (1 - beta), on the step at most half
    that (the step goes with 1 / sqrt(v))."""
    for beta in (0.9, 0.999):
        ours, torchs = 1.0 - float(f32(beta)), 1.0 - beta
        rel = abs(ours - torchs) / torchs
        print(f"beta {beta}: 1 - beta {ours!r} against {torchs!r}, {rel:.3e} relative (limit {2.0 ** -24 / torchs:.3e})")
        assert rel <= 2.0 ** -24 / torchs
        assert abs(np.sqrt(torchs / ours) - 1.0) <= 0.5 * 2.0 ** -24 / torchs * (1 + 1e-4)
    assert abs(abs(1.0 - float(f32(0.999)) - 0.001) / 0.001 - 1.3e-5) < 1e-6
