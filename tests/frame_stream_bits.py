"""The cases behind tests/golden/frame_stream_parent_bits.npz (test code only): seeded inputs and one function that runs the
streaming kernels around the frame solve on the GPU -- csrc/frame_vjp.hip, frame_sizing_grad.hip, frame_loads.hip, seven C
entries called directly -- and returns every output as raw bits.  tests/golden/make_frame_stream_parent_bits.py records them, and
tests/test_gpu_frame_stream_bits.py compares a later build with the record: stating the node walk, the end-node contraction and
the streaming launch once must not move a bit.

There is no solve between the kernels (the band solve's assembly is not under test): disp, lambda, V, M, the forces and the
cotangents are seeded arrays of realistic magnitude.  Every output buffer starts as SENTINEL, so rows that must not be written are
compared too.  B = 7 frames per case:

  g1x1   grid 1 x 1,  Nn  4   frame_sizing_rhs_kernel<4>, 16 frames to a wave: a partly filled wave
  g1x3   grid 1 x 3,  Nn  8   <8>
  g2x3   grid 2 x 3,  Nn 12   <16> with idle lanes
  hub    hub_frame,   Nn 19   <32>; a node with 18 incident ends (the walk's long list)
  brace  custom_frame(2, 2, pinned, braced), Nn 9   inclined elements (c and s both non-zero), pinned bases
  g6x5   grid 6 x 5,  Nn 42   <64>
  g10x6  grid 10 x 6, Nn 77   <64> with two nodes per lane
  big    the inputs of g10x6 tiled to B = 7000: 539 000 node rows, more than one pass of the 2048 x 256 grid.  Its record is the
         first seven frames' rows, and `replicas` counts the entries of the other 999 replicas that differ from them

Frame 3 is inactive (the sizing entries), frame 5 failed in the forward and frame 1 in the adjoint solve (the entries that take a
status).  Runs per case, "<entry>_<variant>": the cotangent entries with every cotangent (`all`) and with gM alone (`gM`); the load
entries with per-frame strides (`pf`) and with both strides 0 (`sh`; ops_frame_load_vjp_f64 takes no stride); the sizing right-hand
side with both hinges (`hinge`: the limits are the medians of |ux| and |uy|, so both branches of each run) and with both alphas 0
and no loss_extra (`plain`)."""
import ctypes

import numpy as np

SEED = 20261019
B = 7
REPLICAS = 1000
SENTINEL = -12345.678
INACTIVE, FAILED_FWD, FAILED_ADJ = 3, 5, 1
ALPHA_SWAY, ALPHA_DEFLECTION = 0.5, 0.25
GRIDS = {"g1x1": (1, 1), "g1x3": (1, 3), "g2x3": (2, 3), "g6x5": (6, 5), "g10x6": (10, 6)}
CASES = ("g1x1", "g1x3", "g2x3", "hub", "brace", "g6x5", "g10x6", "big")
NODES = {"g1x1": 4, "g1x3": 8, "g2x3": 12, "hub": 19, "brace": 9, "g6x5": 42, "g10x6": 77, "big": 77}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def topology(case, device):
    from openpystruct_amd import frames
    from tests import frame_dense
    if case == "hub":
        return frame_dense.hub_frame(device)
    if case == "brace":
        return frame_dense.custom_frame(2, 2, True, True, device)
    return frames.grid_frame(*GRIDS["g10x6" if case == "big" else case], device=device)


def inputs(case, Nn, Ne):
    """Seeded host arrays of one case, B frames ("big": those of g10x6, tiled)."""
    from tests import frame_dense
    if case == "big":
        return {k: np.tile(z, (REPLICAS,) + (1,) * (z.ndim - 1)) for k, z in inputs("g10x6", Nn, Ne).items()}
    rng = np.random.default_rng([SEED, CASES.index(case)])
    n = rng.standard_normal
    x = dict(I=frame_dense.random_inertias(rng, B, Ne), disp=1e-3 * n((B, Nn, 3)), lam=1e-6 * n((B, Nn, 3)),
             V=1e4 * n((B, Ne)), M=1e4 * n((B, Ne)), forces=1e4 * n((B, Ne, 6)), g_disp=n((B, Nn, 3)), g_forces=n((B, Ne, 6)),
             gV=n((B, Ne)), gM=n((B, Ne)), loads=1e4 * n((B, Nn, 3)), w=1e4 * n((B, Ne, 2)))
    x["active"] = np.ones(B, dtype=np.uint8); x["active"][INACTIVE] = 0
    x["status_fwd"] = np.zeros(B, dtype=np.int32); x["status_fwd"][FAILED_FWD] = 1
    x["status_adj"] = np.zeros(B, dtype=np.int32); x["status_adj"][FAILED_ADJ] = 1
    return x


def _run_case(lib, torch, case):
    from openpystruct_amd import _cabi, frames
    dev = torch.device("cuda")
    topo = topology(case, dev)
    Nn, Ne = topo.Nn, topo.Ne
    assert Nn == NODES[case], (case, Nn)
    x = inputs(case, Nn, Ne)
    nb = x["I"].shape[0]
    ux, uy = np.abs(x["disp"][:B, :, 0]), np.abs(x["disp"][:B, :, 1])
    s_lim, d_lim = float(np.median(ux)), float(np.median(uy))
    for a, lim in ((ux, s_lim), (uy, d_lim)):      # both branches of each hinge run
        assert (a > lim).any() and (a < lim).any(), case
    d = {k: torch.as_tensor(z).to(dev) for k, z in x.items()}
    adj = frames._adjoint_tables(topo)
    hp = frames._sizing_params(frames.FrameConfig())
    hinge = _cabi.FrameSizingObjective(alpha_sway=ALPHA_SWAY, sway_limit=s_lim, alpha_deflection=ALPHA_DEFLECTION, deflection_limit=d_lim)
    plain = _cabi.FrameSizingObjective(alpha_sway=0.0, sway_limit=0.0, alpha_deflection=0.0, deflection_limit=0.0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    geo, EA, E = topo.d_geo.data_ptr(), topo.d_EA.data_ptr(), topo.d_E.data_ptr()
    conn, ptr, idx = adj.conn.data_ptr(), adj.ptr.data_ptr(), adj.idx.data_ptr()
    p = {k: t.data_ptr() for k, t in d.items()}
    out = {}

    def new(name, *shape):
        out[name] = torch.full((nb,) + shape, SENTINEL, dtype=torch.float64, device=dev)
        return out[name].data_ptr()

    def ok(rc, what):
        assert rc == 0, (case, what, rc)

    for v, (g_disp, g_forces, gV) in (("all", (p["g_disp"], p["g_forces"], p["gV"])), ("gM", (None, None, None))):
        ok(lib.ops_frame_adjoint_rhs_f64(nb, Nn, Ne, geo, EA, E, conn, ptr, idx, p["I"], g_disp, g_forces, gV, p["gM"],
                                         new("adjoint_rhs_" + v, Nn, 3), stream), "adjoint_rhs")
        ok(lib.ops_frame_grad_contract_f64(nb, Nn, Ne, geo, E, conn, p["disp"], p["lam"], g_forces, gV, p["gM"], p["status_fwd"],
                                           p["status_adj"], new("grad_contract_" + v, Ne), stream), "grad_contract")
        ok(lib.ops_frame_load_vjp_f64(nb, Nn, Ne, geo, conn, p["lam"], g_forces, gV, p["gM"], p["status_fwd"], p["status_adj"],
                                      new("load_vjp_" + v, Ne, 2), stream), "load_vjp")
    ok(lib.ops_frame_sizing_rhs_f64(nb, Nn, Ne, geo, EA, E, ptr, idx, p["I"], p["disp"], p["V"], p["M"], ctypes.byref(hp),
                                    ctypes.byref(hinge), p["active"], new("sizing_rhs_hinge", Nn, 3), new("sizing_extra_hinge"),
                                    stream), "sizing_rhs")
    ok(lib.ops_frame_sizing_rhs_f64(nb, Nn, Ne, geo, EA, E, ptr, idx, p["I"], p["disp"], p["V"], p["M"], ctypes.byref(hp),
                                    ctypes.byref(plain), p["active"], new("sizing_rhs_plain", Nn, 3), None, stream), "sizing_rhs")
    ok(lib.ops_frame_sizing_grad_f64(nb, Nn, Ne, geo, E, conn, p["I"], p["disp"], p["V"], p["M"], p["lam"], ctypes.byref(hp),
                                     p["active"], p["status_fwd"], p["status_adj"], new("sizing_grad", Ne), stream), "sizing_grad")
    for v, lbs, wbs in (("pf", 3 * Nn, 2 * Ne), ("sh", 0, 0)):
        ok(lib.ops_frame_load_rhs_f64(nb, Nn, Ne, geo, ptr, idx, p["loads"], lbs, p["w"], wbs, new("load_rhs_" + v, Nn, 3), stream),
           "load_rhs")
        out["load_forces_" + v] = d["forces"].clone()
        ok(lib.ops_frame_load_forces_f64(nb, Ne, geo, p["w"], wbs, p["status_fwd"], out["load_forces_" + v].data_ptr(),
                                         new("load_V_" + v, Ne), new("load_M_" + v, Ne), stream), "load_forces")
    torch.cuda.synchronize()
    got = {}
    if case == "big":      # every replica against the first, on the GPU; the record is the first replica
        diff = 0
        for t in out.values():
            r = t.view(torch.int64).reshape(REPLICAS, -1)
            diff += int((r != r[:1]).sum())
        got["replicas"] = np.array([diff], dtype=np.uint64)
    got.update({k: bits(t[:B].cpu().numpy()) for k, t in out.items()})
    return got


def run_all():
    """Every case on the GPU: {case: {array: raw bits}}."""
    import torch

    from openpystruct_amd import _cabi
    lib = _cabi.load()
    return {case: _run_case(lib, torch, case) for case in CASES}
