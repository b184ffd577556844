"""tests/frame_dense.py's dense float64 model with the element loads as an argument (test code only): beamUniform (wy, wx) per
element and per frame enters as a differentiable torch tensor, so autograd of this model is the reference for the gradient with
respect to the element loads (csrc/frame_loads.hip).  Runs on the CPU."""
import numpy as np
import torch

from tests import frame_dense as fd


def load_directions(case: fd.FrameCase):
    """(Dy, Dx) [Ne,6] each: the consistent global end loads of a unit wy and of a unit wx; pg_e = wy_e Dy_e + wx_e Dx_e."""
    Ne = case.conn.shape[0]
    Dy, Dx = np.zeros((Ne, 6)), np.zeros((Ne, 6))
    for e in range(Ne):
        d = case.coords[case.conn[e, 1]] - case.coords[case.conn[e, 0]]
        L = float(np.hypot(d[0], d[1]))
        c, s = d[0] / L, d[1] / L
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        T = np.zeros((6, 6)); T[:3, :3] = R; T[3:, 3:] = R
        Dy[e] = T.T @ np.array([0.0, L / 2, L * L / 12, 0.0, L / 2, -L * L / 12])
        Dx[e] = T.T @ np.array([L / 2, 0.0, 0.0, L / 2, 0.0, 0.0])
    return Dy, Dx


def dense_frame_solve_w(case: fd.FrameCase, I: torch.Tensor, loads: torch.Tensor, w: torch.Tensor):
    """I [B,Ne], loads [Nn,3] | [B,Nn,3], w [Ne,2] | [B,Ne,2] (wy, wx; the case's own wy / wx are NOT used), float64 torch ->
    disp [B,Nn,3], forces [B,Ne,6], V, M [B,Ne]."""
    B, Ne = I.shape
    Nn = case.coords.shape[0]
    Kax, Kb, _, dofs = fd._element_matrices(case)
    Kax, Kb, dofs = torch.tensor(Kax), torch.tensor(Kb), torch.tensor(dofs)
    Dy, Dx = (torch.tensor(a) for a in load_directions(case))
    w = w.expand(B, Ne, 2)
    pg = w[..., 0:1] * Dy + w[..., 1:2] * Dx                                # [B,Ne,6]
    Ke = Kax + I[:, :, None, None] * Kb
    bi = torch.arange(B)[:, None].expand(B, Ne)
    K = torch.zeros(B, 3 * Nn, 3 * Nn, dtype=torch.float64)
    for a in range(6):
        for c in range(6):
            K = K.index_put((bi, dofs[:, a].expand(B, Ne), dofs[:, c].expand(B, Ne)), Ke[:, :, a, c], accumulate=True)
    f = loads.expand(B, Nn, 3).reshape(B, 3 * Nn)
    for a in range(6):
        f = f.index_put((bi, dofs[:, a].expand(B, Ne)), pg[:, :, a], accumulate=True)
    d = torch.tensor(~np.asarray(case.fix3, dtype=bool).reshape(-1), dtype=torch.float64)
    Kc = K * d[:, None] * d[None, :] + torch.diag(1.0 - d)
    u = torch.cholesky_solve((f * d)[..., None], torch.linalg.cholesky(Kc))[..., 0]
    ue = u[:, dofs]
    forces = (Ke @ ue[..., None])[..., 0] - pg
    return u.reshape(B, Nn, 3), forces, forces[..., 1], forces[..., 2]


def random_element_loads(rng, B, Ne, zero_frame=None):
    """Distinct wy and wx on every element (columns and braces included), ~1e4 N/m; frame `zero_frame` gets none at all."""
    w = rng.uniform(0.3, 2.0, size=(B, Ne, 2)) * rng.choice([-1.0, 1.0], size=(B, Ne, 2)) * 1e4
    if zero_frame is not None:
        w[zero_frame] = 0.0
    return w

