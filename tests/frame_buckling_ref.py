"""Dense float64 reference of the linear buckling load factors of a frame (test code only, runs on the CPU): the
dense K from tests/frame_dense.py::_element_matrices, the dense S = -K_g(N) from this file's own statement of the geometric
matrices and the axial forces of tests/frame_dense.py::dense_frame_solve, mu as eigh(L^-1 S_ff L^-T) descending (K_ff = L L^T), a
NumPy restatement of the iteration of csrc/frame_buckling.hpp from the same start, and the gradient as torch autograd of the
dense model (dense_frame_solve -> N -> eigvalsh), which knows nothing of the adjoint formula.  Also the cases, inputs and
constants the host tests (tests/test_frame_buckling_host.py) and the GPU tests (tests/test_gpu_frame_buckling.py) share."""
import functools

import numpy as np
import torch

from tests import frame_dense as fd
from tests.frame_modes_ref import EPS, default_start, dense_K, fix_sign, free_dofs, topology  # noqa: F401

ITERS = 16           # the converged run of the GPU tests
GAP = 0.25           # mode 2 is compared where its relative gap to both neighbours is at least this


def unit_geometric_matrices(case, kind):
    """([Ne,6,6] global k_g,unit (the geometric matrix at N = 1), [Ne,6] the weights of the end forces in N)."""
    Ne = case.conn.shape[0]
    out, ax = np.zeros((Ne, 6, 6)), np.zeros((Ne, 6))
    for e in range(Ne):
        d = case.coords[case.conn[e, 1]] - case.coords[case.conn[e, 0]]
        L = float(np.hypot(d[0], d[1]))
        c, s = d[0] / L, d[1] / L
        if kind == "consistent":
            k4 = np.array([[36, 3 * L, -36, 3 * L], [3 * L, 4 * L * L, -3 * L, -L * L], [-36, -3 * L, 36, -3 * L],
                           [3 * L, -L * L, -3 * L, 4 * L * L]]) / (30 * L)
        else:
            k4 = np.zeros((4, 4))
            k4[0, 0] = k4[2, 2] = 1 / L
            k4[0, 2] = k4[2, 0] = -1 / L
        k = np.zeros((6, 6))
        k[np.ix_([1, 2, 4, 5], [1, 2, 4, 5])] = k4
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        T = np.zeros((6, 6)); T[:3, :3] = R; T[3:, 3:] = R
        out[e] = T.T @ k @ T
        ax[e] = (-c / 2, -s / 2, 0.0, c / 2, s / 2, 0.0)
    return out, ax


def dense_S(case, N, kgu):
    """[3 Nn, 3 Nn]: -sum_e N_e k_g,unit,e."""
    _, _, _, dofs = fd._element_matrices(case)
    n = 3 * case.coords.shape[0]
    S = np.zeros((n, n))
    for e in range(len(N)):
        S[np.ix_(dofs[e], dofs[e])] -= N[e] * kgu[e]
    return S


def abs_S(case, forces, kgu, ax):
    """[3 Nn, 3 Nn]: sum_e (|ax_e| . |f_e|) |k_g,unit,e|, the size of the terms an entry of S is a sum of."""
    return -dense_S(case, (np.abs(ax) * np.abs(forces)).sum(-1), np.abs(kgu))


def static_forces(case, I, loads=None):
    """[Ne,6]: the end forces of the dense static solve of one frame (I [Ne]; loads [Nn,3], None: the case's own)."""
    with torch.no_grad():
        return fd.dense_frame_solve(case, torch.tensor(I)[None], None if loads is None else torch.tensor(loads))[1][0].numpy()


def dense_buckling(case, I, S):
    """(mu [n_eq] descending, phi [n_eq, 3 Nn] with phi^T K phi = 1, zero on constrained DOFs, largest component positive) of
    S phi = mu K phi."""
    f = free_dofs(case)
    Lc = np.linalg.cholesky(dense_K(case, I)[np.ix_(f, f)])
    C = np.linalg.solve(Lc, np.linalg.solve(Lc, S[np.ix_(f, f)]).T)
    mu, Y = np.linalg.eigh((C + C.T) / 2)
    mu, Y = mu[::-1], Y[:, ::-1]
    phi = np.zeros((len(f), S.shape[0]))
    phi[:, f] = np.linalg.solve(Lc.T, Y).T
    return mu, fix_sign(phi)


def load_factors(mu):
    with np.errstate(divide="ignore"):
        return np.where(mu > 0.0, 1.0 / np.where(mu > 0.0, mu, 1.0), np.inf)


def gap(mu, j):
    """Relative gap of mu_j (descending, at least j + 2 values) to its nearer neighbour."""
    g = (mu[j] - mu[j + 1]) / abs(mu[j])
    return float(g if j == 0 else min(g, (mu[j - 1] - mu[j]) / abs(mu[j])))


def ritz_step(X, SX, R):
    """One Ritz step on rows X, SX, R [p, n] -> (mu [p] descending, Q [p,n], R_next [p,n], Kr); LinAlgError when X K X^T is not positive
    definite."""
    Kr = X @ R.T
    Kr = (Kr + Kr.T) / 2
    Sr = X @ SX.T
    Sr = np.triu(Sr) + np.triu(Sr, 1).T
    G = np.linalg.cholesky(Kr)
    A = np.linalg.solve(G, np.linalg.solve(G, Sr).T)
    mu, V = np.linalg.eigh((A + A.T) / 2)
    mu, V = mu[::-1], V[:, ::-1]
    Z = np.linalg.solve(G.T, V)
    return mu, Z.T @ X, Z.T @ SX, Kr


def iterate(case, I, S, X0, iters):
    """The iteration from X0 [p, 3 Nn]: a list of (mu, Q, R_next, X, SX, R, Kr) per iteration (X, SX, R: what the Ritz step was given,
    R = S X0 at the start)."""
    f = free_dofs(case)
    Lc = np.linalg.cholesky(dense_K(case, I)[np.ix_(f, f)])
    R = X0 @ S.T
    out = []
    for _ in range(iters):
        X = np.zeros_like(R)
        X[:, f] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, R[:, f].T)).T
        SX = X @ S.T
        mu, Q, Rn, Kr = ritz_step(X, SX, R)
        out.append((mu, Q, Rn, X, SX, R, Kr))
        R = Rn
    return out


def autograd_gradient(case, I, loads, kind, g):
    """(lambda [2], sum_j g_j dlambda_j/dI [Ne]) of the two lowest load factors by torch autograd through the dense model: the static
    solve, the axial forces, the dense pencil and eigvalsh.  A load factor of +inf takes no part."""
    kgu, ax = unit_geometric_matrices(case, kind)
    Kax, Kb, _, dofs = fd._element_matrices(case)
    It = torch.tensor(I, requires_grad=True)
    forces = fd.dense_frame_solve(case, It[None], None if loads is None else torch.tensor(loads))[1][0]
    N = (forces * torch.tensor(ax)).sum(-1)
    n = 3 * case.coords.shape[0]
    K, S = torch.zeros(n, n, dtype=torch.float64), torch.zeros(n, n, dtype=torch.float64)
    for e in range(len(I)):
        ix = np.ix_(dofs[e], dofs[e])
        K[ix] = K[ix] + torch.tensor(Kax[e]) + It[e] * torch.tensor(Kb[e])
        S[ix] = S[ix] - N[e] * torch.tensor(kgu[e])
    f = free_dofs(case)
    Lc = torch.linalg.cholesky(K[np.ix_(f, f)])
    C = torch.linalg.solve_triangular(Lc, S[np.ix_(f, f)], upper=False)
    C = torch.linalg.solve_triangular(Lc, C.T, upper=False)
    mu = torch.linalg.eigvalsh((C + C.T) / 2).flip(0)[:2]
    lam = torch.where(mu > 0.0, 1.0 / mu, torch.full_like(mu, np.inf))
    loss = sum(float(g[j]) * lam[j] for j in range(2) if float(mu[j].detach()) > 0.0)
    grad = torch.autograd.grad(loss, It)[0].numpy() if torch.is_tensor(loss) else np.zeros(len(I))
    return lam.detach().numpy(), grad


# ---- the cases the host and the GPU tests share ----
# name: topology, B, kind, load state ("own": the topology's loads, the factor's keeping solution; "case": one frame_resolve case
# with per-frame nodal loads and the topology's element loads), vectors
CASES = {
    "1x1-c": ("1x1", 5, "consistent", "own", 3),
    "3x6-p": ("3x6", 1, "pdelta", "own", 8),
    "3x6-c": ("3x6", 5, "consistent", "own", 8),
    "10x4n-c": ("10x4n", 67, "consistent", "own", 8),
    "general-c": ("general", 5, "consistent", "case", 8),
    "hub-p": ("hub", 5, "pdelta", "own", 8),
}
# Inertias within this factor of 5e-4 instead of fd.random_inertias' two decades, where the NumPy restatement of the iteration does
# not meet the conditions of tests/test_frame_buckling_host.py::test_conditions_of_the_gpu_cases in ITERS iterations on the case's
# vectors.  The rate of mode j is |mu_(p+1)| / mu_j, the negative mu of tensioned members among them.  Over two decades: 1x1-c (three
# vectors) leaves the second shape at 6.4e-7; 3x6-c at 1.2e-8; on 10x4n-c the ninth |mu| exceeds the second mu and mode 2 does not
# converge at all, within a factor of 2 its mu stands at 6.7e-10, and however narrow the range |mu_9| / mu_2 stays above 0.31, so the
# second shape of the ten-bay frame is at 1.1e-8 after ITERS iterations (SHAPE_ERROR below).
SPREAD = {"1x1-c": 4.0, "3x6-c": 4.0, "10x4n-c": 1.1}


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(case, I [B,Ne], loads [B,Nn,3] | None, kind, p) of a shared case.  Inertias from fd.random_inertias, log-uniform over two
    decades, except where SPREAD names a narrower range."""
    name, B, kind, state, p = CASES[key]
    case = fd.case_of(topology(name, "cpu"))
    Nn, Ne = case.coords.shape[0], case.conn.shape[0]
    rng = np.random.default_rng(sum(map(ord, key)) + 31 * B)
    I = fd.random_inertias(rng, B, Ne)
    if key in SPREAD:
        I = 5e-4 * np.exp(rng.uniform(-np.log(SPREAD[key]), np.log(SPREAD[key]), size=(B, Ne)))
    loads = None
    if state == "case":       # gravity on every free node, a lateral push on the left column, both varied per frame
        loads = np.zeros((B, Nn, 3))
        loads[:, :, 1] = -6e4 * rng.uniform(0.5, 1.5, size=(B, Nn))
        loads[:, case.coords[:, 0] == 0.0, 0] = 1e4 * rng.uniform(0.5, 1.5, size=(B, 1))
        loads[:, np.asarray(case.fix3).all(axis=1)] = 0.0
        loads.setflags(write=False)
    I.setflags(write=False)
    return case, I, loads, kind, p


@functools.lru_cache(maxsize=None)
def reference(key):
    """Per frame of a shared case: dict(forces [Ne,6], S, Sabs, mu [n_eq], lam [n_eq], phi [2, 3 Nn], its [ITERS entries of iterate()])."""
    case, I, loads, kind, p = inputs(key)
    kgu, ax = unit_geometric_matrices(case, kind)
    out = []
    for b in range(I.shape[0]):
        forces = static_forces(case, I[b], None if loads is None else loads[b])
        S = dense_S(case, (forces * ax).sum(-1), kgu)
        mu, phi = dense_buckling(case, I[b], S)
        its = iterate(case, I[b], S, default_start(case, p), ITERS)
        out.append(dict(forces=forces, S=S, Sabs=abs_S(case, forces, kgu, ax), mu=mu, lam=load_factors(mu), phi=phi[:2], its=its))
    return out


# The converged shapes against dense, K-norm x min(1, gap) on the compared modes: what the NumPy restatement of the iteration itself
# shows after ITERS iterations (the CPU measurement of a converged value; tests/test_frame_buckling_host.py pins it).  Where it is at
# most 1e-10 the GPU bound is the project's 1e-8, otherwise 100 x the measurement.  Cases not named measure at most 2e-14.
SHAPE_ERROR = {"3x6-c": 1.2e-9, "10x4n-c": 1.2e-8}


def shape_bound(key):
    return 100.0 * SHAPE_ERROR[key] if key in SHAPE_ERROR else 1e-8


def shape_error(K, got, want):
    """K-norm of the difference of two shapes [3 Nn] up to sign."""
    return float(min(np.sqrt(max((got - s * want) @ K @ (got - s * want), 0.0)) for s in (1.0, -1.0)))


def gradient_frames(key):
    """The frames whose reference gradient is computed (autograd of the dense model costs a dense solve and an eigh per frame): all
    of them up to eight, else the first two, the middle one and the last three (the last wave's tail)."""
    B = CASES[key][1]
    return list(range(B)) if B <= 8 else [0, 1, B // 2, B - 3, B - 2, B - 1]


@functools.lru_cache(maxsize=None)
def reference_gradient(key):
    """(want [F, Ne], g [B, 2], gaps [F]) on F = gradient_frames(key): sum_j g_j dlambda_j/dI by autograd of the dense model, g =
    grad_cotangent(key) with the cotangent of mode 2 zeroed where its gap is below GAP (in every frame, computed or not), and the
    min(1, gap) of the modes that take part."""
    case, I, loads, kind, _ = inputs(key)
    ref, g = reference(key), grad_cotangent(key).copy()
    for b in range(I.shape[0]):
        if gap(ref[b]["mu"], 1) < GAP:
            g[b, 1] = 0.0
    out, gaps = [], []
    for b in gradient_frames(key):
        mu = ref[b]["mu"]
        two = gap(mu, 1) >= GAP
        gaps.append(min([1.0, gap(mu, 0)] + ([gap(mu, 1)] if two else [])))
        out.append(autograd_gradient(case, I[b], None if loads is None else loads[b], kind, g[b])[1])
    return np.stack(out), g, np.array(gaps)


# Constants of the elementwise GPU bounds |got - ref| <= c 2^-52 scale: c = 4 x the largest ratio the g++ build of
# csrc/frame_buckling.hpp shows on the same inputs (room for another order of the same sums).  The ratios as measured, written to
# two decimals rounded up -- geometric apply 2.01036, gradient rows 3.67196; tests/test_frame_buckling_host.py holds the build to them
# from both sides.
GEOM_RATIO, BGRAD_RATIO = 2.02, 3.68
C_GEOM, C_BGRAD = 4.0 * GEOM_RATIO, 4.0 * BGRAD_RATIO


@functools.lru_cache(maxsize=None)
def geom_apply_x(key):
    """[B, 3, 3 Nn]: three rows per frame for the geometric apply alone (values on constrained DOFs too: S is applied as it stands)."""
    case, I, *_ = inputs(key)
    x = np.random.default_rng(len(key) + 7).standard_normal((I.shape[0], 3, 3 * case.coords.shape[0]))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def grad_cotangent(key):
    """[B, 2]: the cotangent of the two lowest load factors."""
    g = np.random.default_rng(len(key) + 11).standard_normal((inputs(key)[1].shape[0], 2))
    g.setflags(write=False)
    return g


def grad_rows(case, kind, phi, lam, g):
    """The reference of ops_frame_buckling_grad_f64 for one frame, phi [m, 3 Nn], lam, g [m]: (direct [Ne], g_forces [Ne,6], and the
    sums of the absolute terms of both)."""
    _, Kb, _, dofs = fd._element_matrices(case)
    kgu, ax = unit_geometric_matrices(case, kind)
    fin = np.isfinite(lam)
    pe, l, g = phi[fin][:, dofs], lam[fin], g[fin]
    direct = np.einsum("j,jea,eab,jeb->e", g * l, pe, Kb, pe)
    a = np.einsum("j,jea,eab,jeb->e", g * l * l, pe, kgu, pe)
    s_direct = np.einsum("j,jea,eab,jeb->e", np.abs(g * l), np.abs(pe), np.abs(Kb), np.abs(pe))
    s_a = np.einsum("j,jea,eab,jeb->e", np.abs(g) * l * l, np.abs(pe), np.abs(kgu), np.abs(pe))
    return direct, a[:, None] * ax, s_direct, s_a[:, None] * np.abs(ax)


def column(n_el, load=-1.0, device="cpu"):
    """A fixed-base vertical cantilever column of 4 m, E = 200e9, A = 0.02, under a vertical tip load (negative: compression)."""
    from openpystruct_amd import frames
    H = 4.0
    coords = np.stack([np.zeros(n_el + 1), np.linspace(0.0, H, n_el + 1)], 1)
    conn = np.stack([np.arange(n_el), np.arange(1, n_el + 1)], 1)
    fix3 = np.zeros((n_el + 1, 3), dtype=bool); fix3[0] = True
    loads = np.zeros((n_el + 1, 3)); loads[n_el, 1] = load
    return frames.FrameTopology(coords, conn, fix3, 0.02, 200e9, np.zeros(n_el), np.zeros(n_el), loads, device)
