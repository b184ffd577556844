"""Dense float64 model of the batched beam solve in plain torch (test code only): assembles K and f, solves the
constrained system, recovers V and M the way csrc/beam_math.hpp's seg_solve does.  Every step is a differentiable torch
operation, so autograd of this model is the reference the beam-solve VJP is checked against.  Runs on the CPU."""
import numpy as np
import torch


def _per_elem(t, B, Ne):
    t = torch.as_tensor(t, dtype=torch.float64)
    return t.reshape(()).expand(B, Ne) if t.numel() == 1 else t


def dense_solve(x, E, I, fix, Fy, wy):
    """x [N] | [B,N], E scalar | [B,Ne], I [B,Ne], fix [N] | [B,N] (uint8 bits), Fy [B,N], wy scalar | [B,Ne]
    -> v, theta [B,N], V, M [B,Ne]."""
    B, Ne = I.shape
    N = Ne + 1
    x = torch.as_tensor(x, dtype=torch.float64).expand(B, N)
    E = _per_elem(E, B, Ne)
    wy = _per_elem(wy, B, Ne)
    fix = torch.as_tensor(np.asarray(fix), dtype=torch.int64).expand(B, N)
    L = x[:, 1:] - x[:, :-1]
    EI = E * I
    kA, kB, kC, kD = 12 * EI / L ** 3, 6 * EI / L ** 2, 4 * EI / L, 2 * EI / L
    ke = torch.stack([torch.stack([kA, kB, -kA, kB], -1), torch.stack([kB, kC, -kB, kD], -1),
                      torch.stack([-kA, -kB, kA, -kB], -1), torch.stack([kB, kD, -kB, kC], -1)], -2)   # [B,Ne,4,4]
    e = torch.arange(Ne)
    bi = torch.arange(B)[:, None].expand(B, Ne)
    K = torch.zeros(B, 2 * N, 2 * N, dtype=torch.float64)
    for a in range(4):
        for c in range(4):
            K = K.index_put((bi, (2 * e + a).expand(B, Ne), (2 * e + c).expand(B, Ne)), ke[:, :, a, c], accumulate=True)
    pw, mw = 0.5 * wy * L, wy * L * L / 12.0
    f = torch.zeros(B, 2 * N, dtype=torch.float64)
    f = f.index_put((torch.arange(B)[:, None].expand(B, N), (2 * torch.arange(N)).expand(B, N)), Fy, accumulate=True)
    for off, val in ((0, pw), (1, mw), (2, pw), (3, -mw)):
        f = f.index_put((bi, (2 * e + off).expand(B, Ne)), val, accumulate=True)
    d = torch.stack([(fix & 1) == 0, (fix & 2) == 0], -1).reshape(B, 2 * N).to(torch.float64)   # 1 = free DOF
    Kc = K * d[:, :, None] * d[:, None, :] + torch.diag_embed(1.0 - d)
    # K_c is SPD (identity on the fixed DOFs): Cholesky, no pivoting.  (torch.linalg.solve's batched LU also stops working in
    # a process whose framework thread count has been changed and restored, which other tests of the suite do.)
    u = torch.cholesky_solve((f * d)[..., None], torch.linalg.cholesky(Kc))[..., 0]
    ue = torch.stack([u[:, 0:-2:2], u[:, 1:-1:2], u[:, 2::2], u[:, 3::2]], -1)   # [B,Ne,4]
    q = (ke @ ue[..., None])[..., 0]
    return u[:, 0::2], u[:, 1::2], q[..., 0] - pw, q[..., 1] - mw


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
