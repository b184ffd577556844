"""Dense float64 model of the batched frame solve in plain torch (test code only): the arithmetic of
oracle/beam_oracle.py::solve_model_3dof -- rotated ElasticBeam2d stiffness matrices, consistent beamUniform loads, PlainHandler
constraints, global end forces -- with every step a differentiable torch operation, so autograd of this model is the reference
the frame-solve VJP (csrc/frame_vjp.hip) is checked against.  Runs on the CPU.  The role tests/beam_dense.py
plays for the beam solve."""
from typing import NamedTuple

import numpy as np
import torch


class FrameCase(NamedTuple):
    """A topology as plain arrays (what a `frames.FrameTopology` keeps on the host)."""
    coords: np.ndarray     # [Nn,2]
    conn: np.ndarray       # [Ne,2]
    fix3: np.ndarray       # [Nn,3] bool
    A: np.ndarray          # [Ne]
    E: np.ndarray          # [Ne]
    wy: np.ndarray         # [Ne]
    wx: np.ndarray         # [Ne]
    nodal_loads: np.ndarray  # [Nn,3]


def case_of(topo) -> FrameCase:
    return FrameCase(topo.coords, topo.conn, topo.fix3, topo.A, topo.E, topo.wy, topo.wx, topo.nodal_loads)


def _element_matrices(case: FrameCase):
    """Per element: K_ax (the axial part of the rotated stiffness), K_b (the bending part per unit inertia), the consistent
    global loads pg, and the global DOF numbers (3 node + dof) of its six end DOFs."""
    Ne = case.conn.shape[0]
    Kax, Kb, pg = np.zeros((Ne, 6, 6)), np.zeros((Ne, 6, 6)), np.zeros((Ne, 6))
    for e in range(Ne):
        d = case.coords[case.conn[e, 1]] - case.coords[case.conn[e, 0]]
        L = float(np.hypot(d[0], d[1]))
        c, s = d[0] / L, d[1] / L
        R = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        T = np.zeros((6, 6)); T[:3, :3] = R; T[3:, 3:] = R
        ka = np.zeros((6, 6)); ka[0, 0] = ka[3, 3] = 1.0; ka[0, 3] = ka[3, 0] = -1.0
        kb = np.zeros((6, 6))
        k4 = np.array([[12, 6 * L, -12, 6 * L], [6 * L, 4 * L * L, -6 * L, 2 * L * L],
                       [-12, -6 * L, 12, -6 * L], [6 * L, 2 * L * L, -6 * L, 4 * L * L]]) / L ** 3
        kb[np.ix_([1, 2, 4, 5], [1, 2, 4, 5])] = k4
        Kax[e] = T.T @ (ka * (case.E[e] * case.A[e] / L)) @ T
        Kb[e] = T.T @ (kb * case.E[e]) @ T
        wy, wx = case.wy[e], case.wx[e]
        pg[e] = T.T @ np.array([wx * L / 2, wy * L / 2, wy * L * L / 12, wx * L / 2, wy * L / 2, -wy * L * L / 12])
    dofs = np.concatenate([3 * case.conn[:, :1] + np.arange(3), 3 * case.conn[:, 1:] + np.arange(3)], axis=1)      # [Ne,6]
    return Kax, Kb, pg, dofs


def dense_frame_solve(case: FrameCase, I: torch.Tensor, loads: torch.Tensor = None):
    """I [B,Ne] and loads [Nn,3] | [B,Nn,3] (None: the case's nodal loads), float64 torch -> disp [B,Nn,3], forces [B,Ne,6],
    V, M [B,Ne]."""
    B, Ne = I.shape
    Nn = case.coords.shape[0]
    Kax, Kb, pg, dofs = _element_matrices(case)
    Kax, Kb, pg, dofs = torch.tensor(Kax), torch.tensor(Kb), torch.tensor(pg), torch.tensor(dofs)
    if loads is None:
        loads = torch.tensor(case.nodal_loads)
    Ke = Kax + I[:, :, None, None] * Kb                                     # [B,Ne,6,6]
    bi = torch.arange(B)[:, None].expand(B, Ne)
    K = torch.zeros(B, 3 * Nn, 3 * Nn, dtype=torch.float64)
    for a in range(6):
        for c in range(6):
            K = K.index_put((bi, dofs[:, a].expand(B, Ne), dofs[:, c].expand(B, Ne)), Ke[:, :, a, c], accumulate=True)
    f = loads.expand(B, Nn, 3).reshape(B, 3 * Nn)
    for a in range(6):
        f = f.index_put((bi, dofs[:, a].expand(B, Ne)), pg[:, a].expand(B, Ne), accumulate=True)
    d = torch.tensor(~np.asarray(case.fix3, dtype=bool).reshape(-1), dtype=torch.float64)      # 1 = free DOF
    Kc = K * d[:, None] * d[None, :] + torch.diag(1.0 - d)
    u = torch.cholesky_solve((f * d)[..., None], torch.linalg.cholesky(Kc))[..., 0]          # SPD: identity on the constrained DOFs
    ue = u[:, dofs]                                                          # [B,Ne,6]
    forces = (Ke @ ue[..., None])[..., 0] - pg
    return u.reshape(B, Nn, 3), forces, forces[..., 1], forces[..., 2]


def cond_free(case: FrameCase, I) -> float:
    """cond(K_ff) of one frame (I [Ne]): what the rounding error of any elimination order scales with."""
    Kax, Kb, _, dofs = _element_matrices(case)
    Nn = case.coords.shape[0]
    K = np.zeros((3 * Nn, 3 * Nn))
    for e in range(len(I)):
        K[np.ix_(dofs[e], dofs[e])] += Kax[e] + float(I[e]) * Kb[e]
    free = ~np.asarray(case.fix3, dtype=bool).reshape(-1)
    return float(np.linalg.cond(K[np.ix_(free, free)]))


def fold(B, Ne, g_forces, gV, gM):
    """g_f of DESIGN.md §9f [B,Ne,6]: g_forces with gV added to component 1 and gM to component 2 (numpy; None = zero)."""
    gf = np.zeros((B, Ne, 6)) if g_forces is None else np.array(g_forces, dtype=np.float64)
    if gV is not None:
        gf[..., 1] += gV
    if gM is not None:
        gf[..., 2] += gM
    return gf


def gI_term_scale(case: FrameCase, disp, lam, gf) -> float:
    """Norm over the batch of the size of the terms each gI_e = (g_f,e - lambda_e) . (K_b,e u_e) is a sum of,
    sum_k (|g_f| + |lambda|)_k (|K_b| |u|)_k: g_f - lambda can cancel, so the rounding error of gI is bounded relative to this,
    not to |gI|.  disp, lam [B,Nn,3] (lam: dL/dloads per frame), gf [B,Ne,6]."""
    _, Kb, _, dofs = _element_matrices(case)
    B = disp.shape[0]
    ue = np.abs(np.asarray(disp).reshape(B, -1)[:, dofs])                    # [B,Ne,6]
    le = np.abs(np.asarray(lam).reshape(B, -1)[:, dofs])
    y = np.einsum("eac,bec->bea", np.abs(Kb), ue)
    return float(np.linalg.norm(((np.abs(gf) + le) * y).sum(-1)))


def random_inertias(rng, B, Ne):
    """Log-uniform in [5e-5, 5e-3]: the range of tests/test_gpu_frames.py."""
    return np.exp(rng.uniform(np.log(5e-5), np.log(5e-3), size=(B, Ne)))


def custom_frame(bays, stories, pinned, brace, device):
    """The general topology of tests/test_gpu_frames.py (test_general_topologies_vs_oracle): pinned bases, diagonal braces."""
    from openpystruct_amd import frames
    nb1 = bays + 1
    coords = np.array([(j * 4.0, i * 3.0) for i in range(stories + 1) for j in range(nb1)])
    conn = [(i * nb1 + j, (i + 1) * nb1 + j) for i in range(stories) for j in range(nb1)]
    conn += [(i * nb1 + j, i * nb1 + j + 1) for i in range(1, stories + 1) for j in range(bays)]
    if brace:
        conn += [(i * nb1, (i + 1) * nb1 + 1) for i in range(stories)]
    conn = np.array(conn)
    fix3 = np.zeros((coords.shape[0], 3), dtype=bool)
    fix3[coords[:, 1] == 0.0] = (True, True, not pinned)
    if pinned and (int((~fix3).sum()) % 3) == 0:
        fix3[0] = True
    loads = np.zeros((coords.shape[0], 3))
    loads[(coords[:, 0] == 0.0) & (coords[:, 1] != 0.0), 0] = 2.5e4
    loads[-1] = (0.0, -4e4, 1e3)
    w = np.zeros(len(conn)); w[stories * nb1: stories * nb1 + stories * bays] = -1.2e4
    return frames.FrameTopology(coords, conn, fix3, 0.02, 200e9, w, 0.5 * w, loads, device)


def hub_frame(device):
    """The hub of tests/test_gpu_frames.py: a node with eighteen incident elements, in the middle of the numbering."""
    from openpystruct_amd import frames
    nn, hub = 19, 9
    ang = np.linspace(0.0, 2 * np.pi, nn - 1, endpoint=False)
    coords = np.zeros((nn, 2))
    outer = [i for i in range(nn) if i != hub]
    coords[outer, 0], coords[outer, 1] = 5.0 * np.cos(ang), 5.0 * np.sin(ang)
    conn = np.array([(hub, o) for o in outer] + [(outer[i], outer[i + 1]) for i in range(len(outer) - 1)])
    fix3 = np.zeros((nn, 3), dtype=bool)
    fix3[0] = fix3[nn - 1] = True
    loads = np.zeros((nn, 3)); loads[hub] = (3e4, -5e4, 2e3); loads[3] = (0.0, -1e4, 0.0)
    w = np.zeros(len(conn)); w[:4] = -8e3
    return frames.FrameTopology(coords, conn, fix3, 0.02, 200e9, w, 0.5 * w, loads, device, numbering="node")
