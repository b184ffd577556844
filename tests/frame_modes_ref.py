"""Dense float64 reference of the natural frequencies of a frame (test code only, runs on the CPU): the dense K from
tests/frame_dense.py::_element_matrices, the dense M from this file's own statement of the mass matrices, the eigenvalues as
1 / eigh of K_ff^-1 M_ff (largest first: it also serves a singular lumped M), a NumPy restatement of the subspace iteration of
csrc/frame_modes.hpp from the same start, and dlambda/dI from the dense eigenvectors.  Also the cases, inputs and constants the
host tests (tests/test_frame_modes_host.py) and the GPU tests (tests/test_gpu_frame_modes.py) share."""
import functools

import numpy as np

from tests import frame_dense as fd

EPS = 2.0 ** -52
MBAR, NODAL = 157.0, 2000.0


def element_mass_matrices(case, mbar, kind):
    """[Ne,6,6] global element mass matrices of a mass per unit length mbar [Ne]."""
    Ne = case.conn.shape[0]
    out = np.zeros((Ne, 6, 6))
    for e in range(Ne):
        d = case.coords[case.conn[e, 1]] - case.coords[case.conn[e, 0]]
        L = float(np.hypot(d[0], d[1]))
        c, s = d[0] / L, d[1] / L
        if kind == "lumped":
            out[e] = np.diag([mbar[e] * L / 2] * 2 + [0.0] + [mbar[e] * L / 2] * 2 + [0.0])
            continue
        m = np.array([[140, 0, 0, 70, 0, 0], [0, 156, 22 * L, 0, 54, -13 * L], [0, 22 * L, 4 * L * L, 0, 13 * L, -3 * L * L],
                      [70, 0, 0, 140, 0, 0], [0, 54, 13 * L, 0, 156, -22 * L], [0, -13 * L, -3 * L * L, 0, -22 * L, 4 * L * L]]) * (mbar[e] * L / 420)
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        T = np.zeros((6, 6)); T[:3, :3] = R; T[3:, 3:] = R
        out[e] = T.T @ m @ T
    return out


def dense_K(case, I):
    Kax, Kb, _, dofs = fd._element_matrices(case)
    n = 3 * case.coords.shape[0]
    K = np.zeros((n, n))
    for e in range(len(I)):
        K[np.ix_(dofs[e], dofs[e])] += Kax[e] + float(I[e]) * Kb[e]
    return K


def dense_M(case, mbar, kind, nodal=None):
    """[3 Nn, 3 Nn]; nodal [Nn,3] or None."""
    _, _, _, dofs = fd._element_matrices(case)
    n = 3 * case.coords.shape[0]
    M = np.zeros((n, n))
    Me = element_mass_matrices(case, np.broadcast_to(np.asarray(mbar, dtype=np.float64), (case.conn.shape[0],)), kind)
    for e in range(case.conn.shape[0]):
        M[np.ix_(dofs[e], dofs[e])] += Me[e]
    if nodal is not None:
        M[np.arange(n), np.arange(n)] += np.asarray(nodal, dtype=np.float64).reshape(-1)
    return M


def free_dofs(case):
    return np.nonzero(~np.asarray(case.fix3, dtype=bool).reshape(-1))[0]


def dense_modes(case, I, M, n):
    """The n lowest (lambda [n], phi [n, 3 Nn] with phi^T M phi = 1, zero on constrained DOFs, largest component positive) of
    K(I) phi = lambda M phi: K_ff = L L^T, eigh(L^-1 M_ff L^-T) = 1 / lambda, largest first."""
    f = free_dofs(case)
    K = dense_K(case, I)[np.ix_(f, f)]
    Lc = np.linalg.cholesky(K)
    C = np.linalg.solve(Lc, np.linalg.solve(Lc, M[np.ix_(f, f)]).T)
    mu, Y = np.linalg.eigh((C + C.T) / 2)
    mu, Y = mu[::-1][:n], Y[:, ::-1][:, :n]
    phi = np.zeros((n, M.shape[0]))
    phi[:, f] = np.linalg.solve(Lc.T, Y).T
    phi /= np.sqrt(np.einsum("ja,ab,jb->j", phi, M, phi))[:, None]
    return 1.0 / mu, fix_sign(phi)


def fix_sign(phi):
    """The component of largest magnitude positive (the first on a tie); phi [..., n]."""
    lead = np.take_along_axis(phi, np.abs(phi).argmax(-1)[..., None], -1)
    return phi * np.where(lead < 0.0, -1.0, 1.0)


def dlambda_dI(case, phi):
    """[n, Ne]: phi_j,e^T K_b,e phi_j,e for M-normalised phi [n, 3 Nn]."""
    _, Kb, _, dofs = fd._element_matrices(case)
    pe = phi[:, dofs]                                              # [n,Ne,6]
    return np.einsum("jea,eab,jeb->je", pe, Kb, pe)


def grad_scale(case, phi, g):
    """[Ne]: sum_j |g_j| |phi_j,e|^T |K_b,e| |phi_j,e|: the size of the terms a gradient row is a sum of."""
    _, Kb, _, dofs = fd._element_matrices(case)
    pe = np.abs(phi[:, dofs])
    return np.einsum("j,jea,eab,jeb->e", np.abs(g), pe, np.abs(Kb), pe)


def default_start(case, p):
    """X0[j,n,d] = 1 + cos(0.37 (j + 1) (3 n + d + 1)), zero on constrained DOFs; [p, 3 Nn]."""
    n = 3 * case.coords.shape[0]
    x0 = 1.0 + np.cos(0.37 * (np.arange(p, dtype=np.float64)[:, None] + 1.0) * (np.arange(n, dtype=np.float64)[None] + 1.0))
    return np.where(np.asarray(case.fix3, dtype=bool).reshape(-1)[None], 0.0, x0)


def ritz_step(X, MX, R):
    """One Ritz step on rows X, MX, R [p, n] -> (lam [p] ascending, Q [p,n], R_next [p,n]); LinAlgError when X M X^T is not positive
    definite."""
    Kr = X @ R.T
    Kr = (Kr + Kr.T) / 2
    Mr = X @ MX.T
    Mr = np.triu(Mr) + np.triu(Mr, 1).T
    G = np.linalg.cholesky(Mr)
    A = np.linalg.solve(G, np.linalg.solve(G, Kr).T)
    lam, V = np.linalg.eigh((A + A.T) / 2)
    Z = np.linalg.solve(G.T, V)
    return lam, Z.T @ X, Z.T @ MX


def iterate(case, I, M, X0, iters):
    """The subspace iteration from X0 [p, 3 Nn]: a list of (lam, Q, R, X, MX) per iteration (R: the NEXT right-hand side; X, MX: what
    the Ritz step was given, with R_before = the R of the entry before, M X0 at the start)."""
    f = free_dofs(case)
    K = dense_K(case, I)[np.ix_(f, f)]
    Lc = np.linalg.cholesky(K)
    R = X0 @ M.T
    out = []
    for _ in range(iters):
        X = np.zeros_like(R)
        X[:, f] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, R[:, f].T)).T
        MX = X @ M.T
        lam, Q, Rn = ritz_step(X, MX, R)
        out.append((lam, Q, Rn, X, MX, R))
        R = Rn
    return out


def gap(lam, j):
    """Relative gap of eigenvalue j of `lam` (ascending, at least j + 2 values) to its nearer neighbour."""
    g = (lam[j + 1] - lam[j]) / lam[j]
    return float(g if j == 0 else min(g, (lam[j] - lam[j - 1]) / lam[j]))


# ---- the cases the host and the GPU tests share ----
# name: topology, B, mass kind, nodal mass ("none", "shared", "frame"), the vectors of the converged run: min(8, allowed), allowed on
# the 1 x 1 frame (6 equations) 5 with the consistent mass -- with as many vectors as equations the default start is numerically
# dependent after one solve, cond(X^T M X) 1e17 -- and 4 with the lumped one, where four DOFs carry mass
CASES = {
    "1x1-c": ("1x1", 5, "consistent", "shared", 5),
    "1x1-l": ("1x1", 1, "lumped", "none", 4),
    "3x6-l": ("3x6", 5, "lumped", "shared", 8),
    "3x6-c": ("3x6", 1, "consistent", "none", 8),
    "10x4n-c": ("10x4n", 67, "consistent", "frame", 8),
    "general-c": ("general", 5, "consistent", "frame", 8),
    "general-l": ("general", 67, "lumped", "none", 8),
    "hub-c": ("hub", 5, "consistent", "shared", 8),
}
ITERS = 16           # the converged run of the GPU tests
GAP = 0.25           # a mode is compared where its relative gap to both neighbours is at least this


def topology(name, device):
    from openpystruct_amd import frames
    if name == "general":
        return fd.custom_frame(2, 2, True, True, device)
    if name == "hub":
        return fd.hub_frame(device)
    bays, stories = name.rstrip("n").split("x")
    return frames.grid_frame(int(bays), int(stories), device=device, numbering="node" if name.endswith("n") else "auto")


@functools.lru_cache(maxsize=None)
def inputs(key):
    """(case, I [B,Ne], mbar [Ne], nodal [Nn,3] | [B,Nn,3] | None, kind, p) of a shared case: log-uniform inertias, 157 kg/m members
    (x 0.5 .. 2 per element), 2000 kg nodal masses (x 0.5 .. 1.5) on the translations and 50 kg m^2 on the rotation."""
    name, B, kind, nodal_kind, p = CASES[key]
    case = fd.case_of(topology(name, "cpu"))
    Nn, Ne = case.coords.shape[0], case.conn.shape[0]
    rng = np.random.default_rng(sum(map(ord, key)) + 31 * B)
    I = fd.random_inertias(rng, B, Ne)
    if name == "10x4n":      # within a factor of two of 5e-4: over two decades the ninth mode of a ten-bay frame comes within a factor of
        # four of the second, and eight vectors then need more than ITERS / 2 iterations for 1e-10 (lambda_2 / lambda_9 to the 16th)
        I = 5e-4 * np.exp(rng.uniform(-np.log(2.0), np.log(2.0), size=(B, Ne)))
    mbar = MBAR * rng.uniform(0.5, 2.0, size=Ne)
    nodal = None
    if nodal_kind != "none":
        nodal = np.concatenate([NODAL * rng.uniform(0.5, 1.5, size=(B, Nn, 2)), np.full((B, Nn, 1), 50.0)], axis=2)
        nodal = nodal[0] if nodal_kind == "shared" else nodal
    for a in (I, mbar) + (() if nodal is None else (nodal,)):
        a.setflags(write=False)
    return case, I, mbar, nodal, kind, p


def nodal_of(nodal, b):
    return None if nodal is None else (nodal if nodal.ndim == 2 else nodal[b])


@functools.lru_cache(maxsize=None)
def reference(key):
    """Per frame of a shared case: dict(lam [p + 1 or n_eq], phi [2, 3 Nn], dl [2, Ne], its [ITERS // 2 entries of iterate()])."""
    case, I, mbar, nodal, kind, p = inputs(key)
    n_eq = len(free_dofs(case))
    out = []
    for b in range(I.shape[0]):
        M = dense_M(case, mbar, kind, nodal_of(nodal, b))
        lam, phi = dense_modes(case, I[b], M, min(p + 1, n_eq))
        its = iterate(case, I[b], M, default_start(case, p), ITERS // 2)
        out.append(dict(M=M, lam=lam, phi=phi[:2], dl=dlambda_dI(case, phi[:2]), its=its))
    return out


# Constants of the elementwise GPU bounds |got - ref| <= c 2^-52 scale: c = 4 x the largest ratio the g++ build of
# csrc/frame_modes.hpp shows on the same inputs (room for another order of the same sums).  The ratios as measured, written to two
# decimals rounded up -- mass apply 2.6897, gradient 2.5528, both on 10x4n-c; tests/test_frame_modes_host.py holds the build to them
# from both sides.
MASS_RATIO, GRAD_RATIO = 2.69, 2.56
C_MASS, C_GRAD = 4.0 * MASS_RATIO, 4.0 * GRAD_RATIO


@functools.lru_cache(maxsize=None)
def mass_apply_x(key):
    """[B, 3, 3 Nn]: three rows per frame for the mass apply alone (values on constrained DOFs too: M is applied as it stands)."""
    case, I, *_ = inputs(key)
    x = np.random.default_rng(len(key) + 7).standard_normal((I.shape[0], 3, 3 * case.coords.shape[0]))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def grad_cotangent(key):
    """[B, 2]: the cotangent of the two lowest eigenvalues."""
    g = np.random.default_rng(len(key) + 11).standard_normal((inputs(key)[1].shape[0], 2))
    g.setflags(write=False)
    return g


def unit_start(case, p, translations_only=False):
    """[p, 3 Nn]: the unit vectors of the first p free DOFs in node-major order (of the free translations only: the DOFs that carry
    mass under the lumped matrix without nodal masses) -- a start whose first pencil X^T M X is well conditioned even with as many
    vectors as equations, where the default start is numerically dependent after one solve."""
    free = ~np.asarray(case.fix3, dtype=bool)
    if translations_only:
        free = free & np.array([True, True, False])
    idx = np.nonzero(free.reshape(-1))[0][:p]
    assert len(idx) == p
    x0 = np.zeros((p, free.size))
    x0[np.arange(p), idx] = 1.0
    return x0
