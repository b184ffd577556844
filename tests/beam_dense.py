"""Dense float64 model of the batched beam solve in plain torch (test code only): assembles K and f, solves the
constrained system, recovers V and M the way csrc/beam_math.hpp's seg_solve does.  Every step is a differentiable torch
operation, so autograd of this model is the reference the beam-solve VJP is checked against.  Runs on the CPU.
The FE residual r = D (K(I) u - f) and the surrogates' fused residual term (csrc/beam_residual.hip) have element-by-element
float64 references here too (`residual_ref`, `residual_term_ref`): no dense K, so they reach training-size batches."""
import numpy as np
import torch


def _per_elem(t, B, Ne):
    t = torch.as_tensor(t, dtype=torch.float64)
    return t.reshape(()).expand(B, Ne) if t.numel() == 1 else t


def _elements(x, E, I, fix, wy):
    """Element stiffness ke [B,Ne,4,4], consistent UDL loads (pw, mw) [B,Ne] and free-DOF flags (free_v, free_t) [B,N]."""
    B, Ne = I.shape
    N = Ne + 1
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64).expand(B, N)
    E, wy = _per_elem(E, B, Ne), _per_elem(wy, B, Ne)
    fix = torch.as_tensor(np.asarray(fix), dtype=torch.int64).expand(B, N)
    L = x[:, 1:] - x[:, :-1]
    EI = E * I
    kA, kB, kC, kD = 12 * EI / L ** 3, 6 * EI / L ** 2, 4 * EI / L, 2 * EI / L
    ke = torch.stack([torch.stack([kA, kB, -kA, kB], -1), torch.stack([kB, kC, -kB, kD], -1),
                      torch.stack([-kA, -kB, kA, -kB], -1), torch.stack([kB, kD, -kB, kC], -1)], -2)   # [B,Ne,4,4]
    return ke, 0.5 * wy * L, wy * L * L / 12.0, (fix & 1) == 0, (fix & 2) == 0


def _to_nodes(q, N):
    """Scatter per-element end values q [B,Ne,4] (v1, t1, v2, t2) to the nodes: (node v, node theta) [B,N]."""
    B, Ne = q.shape[:2]
    z = torch.zeros(B, N, dtype=q.dtype)
    e1, e2 = torch.arange(Ne), torch.arange(1, N)
    return (z.index_add(1, e1, q[..., 0]).index_add(1, e2, q[..., 2]),
            z.index_add(1, e1, q[..., 1]).index_add(1, e2, q[..., 3]))


def _ends(v, theta):
    return torch.stack([v[:, :-1], theta[:, :-1], v[:, 1:], theta[:, 1:]], -1)     # [B,Ne,4]


def dense_solve(x, E, I, fix, Fy, wy):
    """x [N] | [B,N], E scalar | [B,Ne], I [B,Ne], fix [N] | [B,N] (uint8 bits), Fy [B,N], wy scalar | [B,Ne]
    -> v, theta [B,N], V, M [B,Ne]."""
    B, Ne = I.shape
    N = Ne + 1
    ke, pw, mw, free_v, free_t = _elements(x, E, I, fix, wy)
    e = torch.arange(Ne)
    bi = torch.arange(B)[:, None].expand(B, Ne)
    K = torch.zeros(B, 2 * N, 2 * N, dtype=torch.float64)
    for a in range(4):
        for c in range(4):
            K = K.index_put((bi, (2 * e + a).expand(B, Ne), (2 * e + c).expand(B, Ne)), ke[:, :, a, c], accumulate=True)
    f = torch.zeros(B, 2 * N, dtype=torch.float64)
    f = f.index_put((torch.arange(B)[:, None].expand(B, N), (2 * torch.arange(N)).expand(B, N)), Fy, accumulate=True)
    for off, val in ((0, pw), (1, mw), (2, pw), (3, -mw)):
        f = f.index_put((bi, (2 * e + off).expand(B, Ne)), val, accumulate=True)
    d = torch.stack([free_v, free_t], -1).reshape(B, 2 * N).to(torch.float64)   # 1 = free DOF
    Kc = K * d[:, :, None] * d[:, None, :] + torch.diag_embed(1.0 - d)
    # K_c is SPD (identity on the fixed DOFs): Cholesky, no pivoting.  (torch.linalg.solve's batched LU also stops working in
    # a process whose framework thread count has been changed and restored, which other tests of the suite do.)
    u = torch.cholesky_solve((f * d)[..., None], torch.linalg.cholesky(Kc))[..., 0]
    ue = torch.stack([u[:, 0:-2:2], u[:, 1:-1:2], u[:, 2::2], u[:, 3::2]], -1)   # [B,Ne,4]
    q = (ke @ ue[..., None])[..., 0]
    return u[:, 0::2], u[:, 1::2], q[..., 0] - pw, q[..., 1] - mw


def residual_ref(x, E, I, fix, Fy, wy, v, theta):
    """r = D (K(I) u - f) element by element (no dense K), with the ABI's input forms: x [N] | [B,N], E and wy scalar | [B,Ne],
    fix [N] | [B,N] (bit 1: u_y fixed, bit 2: theta_z fixed), I, v, theta, Fy torch float64 [B,Ne] / [B,N].
    -> (r_v, r_theta, s_v, s_theta) [B,N]: the residual (differentiable in I, v, theta, Fy, E, wy) and, per node, the size of the
    terms it is a sum of, sum_j |ke_ij| |u_j| + |Fy| + |consistent loads| (detached): rounding errors are bounded relative to it."""
    B, Ne = I.shape
    N = Ne + 1
    ke, pw, mw, free_v, free_t = _elements(x, E, I, fix, wy)
    ue = _ends(v, theta)
    Ku_v, Ku_t = _to_nodes((ke @ ue[..., None])[..., 0], N)
    f_v, f_t = _to_nodes(torch.stack([pw, mw, pw, -mw], -1), N)
    f_v = f_v + Fy
    zero = torch.zeros((), dtype=torch.float64)
    rv = torch.where(free_v, Ku_v - f_v, zero)
    rt = torch.where(free_t, Ku_t - f_t, zero)
    with torch.no_grad():
        s_v, s_t = _to_nodes((ke.abs() @ ue.abs()[..., None])[..., 0], N)
        l_v, l_t = _to_nodes(torch.stack([pw, mw, pw, mw], -1).abs(), N)
        s_v, s_t = s_v + l_v + torch.as_tensor(Fy).abs(), s_t + l_t
    return rv, rt, s_v, s_t


def residual_vjp_scales(x, E, I, fix, v, theta, gv, gt):
    """Term sizes of the residual's VJP for the cotangent g = (gv, gt) [B,N], m = D g:  dv, dtheta = K m (per node
    sum_j |ke_ij| |m_j|) and dI_e = m_e^T ke_e u_e / I_e (sum_ij |m_i| |ke_ij| |u_j| / I_e) -> (s_dv, s_dt [B,N], s_dI [B,Ne])."""
    with torch.no_grad():
        ke, _, _, free_v, free_t = _elements(x, E, I, fix, 0.0)
        me = _ends(torch.where(free_v, gv, 0.0).abs(), torch.where(free_t, gt, 0.0).abs())
        s_dv, s_dt = _to_nodes((ke.abs() @ me[..., None])[..., 0], I.shape[1] + 1)
        s_dI = (me[..., None, :] @ ke.abs() @ _ends(v, theta).abs()[..., None])[..., 0, 0] / I
    return s_dv, s_dt, s_dI


def residual_term_ref(preds, nel, sI, disp, rows, Fy, x, E, fix, wy, weight, I_min=1e-8, consts=None):
    """The fused FE-residual term (csrc/beam_residual.hip, header of the fused section) in float64, on the CPU:

        I_e  = clamp(p[b, e] * sI_e + mI_e, I_min)          float32, as the kernels compute the inverse scaler
        u    = recorded (v, theta)[rows[b]]   or   p[b, Ne + n] * s_n + m_n  (float32)
        r    = D (K(I) u - f),  e = r / diag(K(I))          diag and both mean-square scales detached
        term = weight * (mean(e_v^2) / (mean(v^2) + 1e-30) + mean(e_t^2) / (mean(theta^2) + 1e-30))

    Arguments as `physics.fused_residual_term` (preds float32 / bfloat16 [B, >= C]; float64 predictions take the scaler in
    float64).  Returns (term, dpreds, consts): float64 value, d term / d preds [B, C] in float64 (0 where the inertia is
    clamped; C = nel with recorded fields, nel + 2 (nel + 1) with predicted ones) and the detached quantities (diag_v, diag_t,
    mean v^2 + 1e-30, mean theta^2 + 1e-30); `consts` given: those are held at the given values instead."""
    p = preds.detach().cpu()
    dt = torch.float64 if p.dtype == torch.float64 else torch.float32     # float64: the self-check's central differences
    p = p.to(dt)
    B, N = p.shape[0], nel + 1
    recorded = torch.is_tensor(disp[0])
    C = nel if recorded else nel + 2 * N
    p = p[:, :C]
    f32 = lambda t: torch.as_tensor(t).detach().cpu().to(dt)   # noqa: E731
    I32 = p[:, :nel] * f32(sI.scale_)[:nel] + f32(sI.mean_)[:nel]
    I_min32 = torch.tensor(I_min, dtype=dt)
    clamped = I32 < I_min32
    I = torch.where(clamped, I_min32, I32).double().requires_grad_(True)
    r = torch.arange(B) if rows is None else torch.as_tensor(rows).cpu()[:B]
    Fy = torch.as_tensor(Fy).detach().cpu().double()[r]
    if recorded:
        v, t = (torch.as_tensor(d).detach().cpu().double()[r] for d in disp[:2])
    else:
        v = (p[:, nel:nel + N] * f32(disp[0].scale_) + f32(disp[0].mean_)).double().requires_grad_(True)
        t = (p[:, nel + N:] * f32(disp[1].scale_) + f32(disp[1].mean_)).double().requires_grad_(True)
    x, fix = torch.as_tensor(x).detach().cpu(), torch.as_tensor(fix).detach().cpu()
    rv, rt, _, _ = residual_ref(x, E, I, fix, Fy, wy, v, t)
    if consts is None:
        ke = _elements(x, E, I.detach(), fix, 0.0)[0]
        zB = torch.zeros(B, 1, dtype=torch.float64)
        consts = (torch.cat([ke[:, :, 0, 0], zB], 1) + torch.cat([zB, ke[:, :, 2, 2]], 1),
                  torch.cat([ke[:, :, 1, 1], zB], 1) + torch.cat([zB, ke[:, :, 3, 3]], 1),
                  (v.detach() ** 2).mean() + 1e-30, (t.detach() ** 2).mean() + 1e-30)
    d_v, d_t, sc_v, sc_t = consts
    w = float(np.float32(weight))
    term = w * (((rv / d_v) ** 2).mean() / sc_v + ((rt / d_t) ** 2).mean() / sc_t)
    leaves = [I] if recorded else [I, v, t]
    grads = torch.autograd.grad(term, leaves)
    dp = torch.zeros(B, C, dtype=torch.float64)
    dp[:, :nel] = torch.where(clamped, 0.0, grads[0] * f32(sI.scale_)[:nel].double())
    if not recorded:
        dp[:, nel:nel + N] = grads[1] * f32(disp[0].scale_).double()
        dp[:, nel + N:] = grads[2] * f32(disp[1].scale_).double()
    return term.detach(), dp, consts


def cond_free(x, E, I, fix):
    """cond(K_ff) of one beam (x [N], I [Ne], fix [N]): what the rounding error of any elimination order scales with."""
    Ne = len(I)
    x = np.asarray(x, dtype=np.float64)
    L = np.diff(x)
    EI = np.broadcast_to(np.asarray(E, dtype=np.float64) * np.asarray(I, dtype=np.float64), (Ne,))
    K = np.zeros((2 * Ne + 2, 2 * Ne + 2))
    for k in range(Ne):
        l = L[k]
        ke = EI[k] / l ** 3 * np.array([[12, 6 * l, -12, 6 * l], [6 * l, 4 * l * l, -6 * l, 2 * l * l],
                                     [-12, -6 * l, 12, -6 * l], [6 * l, 2 * l * l, -6 * l, 4 * l * l]])
        K[2 * k:2 * k + 4, 2 * k:2 * k + 4] += ke
    fix = np.asarray(fix).astype(np.int64)
    free = np.ones(2 * Ne + 2, dtype=bool); free[0::2] = (fix & 1) == 0; free[1::2] = (fix & 2) == 0
    return float(np.linalg.cond(K[np.ix_(free, free)]))


def random_case(rng, B, Ne, per_beam=False, rz=True):
    """A well-posed random batch: non-uniform mesh, supports at both ends and inside, fixed rotations when `rz`."""
    N = Ne + 1

    def one_mesh():
        return np.sort(rng.uniform(0, 3.0 * Ne, size=N)) + np.arange(N) * 0.5

    def one_fix():
        f = np.zeros(N, dtype=np.uint8)
        f[0] = 3 if (rz or Ne == 1) else 1
        f[-1] = 1
        if N > 4:
            f[rng.integers(1, N - 1)] = 1
        if rz and N > 6:
            f[rng.integers(1, N - 1)] |= 2
        return f

    x = np.stack([one_mesh() for _ in range(B)]) if per_beam else one_mesh()
    fix = np.stack([one_fix() for _ in range(B)]) if per_beam else one_fix()
    I = np.exp(rng.uniform(np.log(1e-2), np.log(0.5), size=(B, Ne)))
    Fy = rng.uniform(-1e5, 1e4, size=(B, N))
    return x, fix, I, Fy


def gI_term_scale(x, I, wy, outs, cot):
    """Size of the largest terms gI is a sum of: every output moves with I like out / I, so no term exceeds
    sum |cot . out| / min I (with the UDL part of V and M counted in full).  gI itself can be far smaller -- for one
    clamped-pinned element V and M do not depend on I at all and gI is a difference of such terms -- so its rounding
    error is bounded relative to this, not to |gI|."""
    v, th, V, M = (np.asarray(o) for o in outs)
    B, Ne = V.shape
    L = np.diff(np.broadcast_to(np.asarray(x, dtype=np.float64), (B, Ne + 1)), axis=-1)
    w = np.broadcast_to(np.asarray(wy, dtype=np.float64), (B, Ne))
    pw, mw = np.abs(0.5 * w * L), np.abs(w * L * L / 12.0)
    s = 0.0
    for o, c, extra in ((v, cot[0], 0.0), (th, cot[1], 0.0), (V, cot[2], pw), (M, cot[3], mw)):
        if c is not None:
            s += float((np.abs(np.asarray(c)) * (np.abs(o) + extra)).sum())
    return s / float(np.min(I))
