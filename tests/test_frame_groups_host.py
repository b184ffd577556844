"""Frame sizing with linked member groups, what needs no GPU: the extension header and its place in the binding and
the build, the package's exports, the refusals the C entry decides before any HIP call, the checks of `member_groups`,
`story_groups` on small grids, `snap_to_catalogue` on hand-written cases, the argument checks of the Python entries, and on the CPU
the chain-rule identity the group step relies on: the segment sum of the per-element gradient at I = X[group] is autograd with one
leaf per group."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "openpystruct_amd_frame_groups.h"
ENTRIES = {"ops_frame_group_step_f32"}
NAMES = ("MemberGroups", "member_groups", "story_groups", "GroupedFrameDesigns", "DiscreteDesigns", "FrameDesignValues",
         "optimize_grouped_frame_designs", "frame_group_gradient", "evaluate_frame_designs", "snap_to_catalogue",
         "generate_grouped_frame_design_dataset")


def test_header_is_an_extension_and_changes_no_version():
    from openpystruct_amd import _cabi, build
    names = [os.path.basename(p) for p in _cabi.EXTENSION_HEADER_PATHS]
    assert HEADER in names
    ext = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index(HEADER)]]
    assert set(ext.functions) == ENTRIES and not ext.structs and not ext.defines
    assert ENTRIES <= set(_cabi.EXTENSION_EXPORTS) and not ENTRIES & set(_cabi.EXPORTS)
    i, p = ctypes.c_int, ctypes.c_void_p
    hp = ctypes.POINTER(_cabi.SizingParams)
    restype, argtypes = ext.functions["ops_frame_group_step_f32"]
    assert restype is i and argtypes == [i] * 5 + [p] * 17 + [i] + [p] * 10 + [hp, p, p]
    # the design step it mirrors: n_groups behind n_elems, the three tables and X behind conn
    design = _cabi._extensions[_cabi.EXTENSION_HEADER_PATHS[names.index("openpystruct_amd_frame_designs.h")]].functions["ops_frame_design_step_f32"]
    assert argtypes == design[1][:4] + [i] + design[1][4:7] + [p] * 4 + design[1][7:]
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "CANNOT VALIDATE" in text and "member_groups" in text
    deps = {os.path.relpath(q, ROOT) for s in build.SOURCES for q in build._deps(s)}      # every file the build watches
    assert os.path.join("include", HEADER) in deps and os.path.join("openpystruct_amd", "csrc", "frame_designs_math.hpp") in deps
    src = os.path.join(ROOT, "openpystruct_amd", "csrc", "frame_groups.hip")
    assert src in build.SOURCES
    scanned = build._deps(src)
    for name in ("frame_designs_math.hpp", "frame_sizing_math.hpp", "sizing_multicase_math.hpp", "lane_common.hpp"):
        assert os.path.normpath(os.path.join(ROOT, "openpystruct_amd", "csrc", name)) in scanned, name
    assert os.path.normpath(os.path.join(ROOT, "include", HEADER)) in scanned
    # one walk for both steps: the design step's source and the group step's call the same function of the math header
    for f in ("frame_designs_math.hpp", "frame_groups.hip"):
        assert "fd_design_walk<K, SUM>(" in open(os.path.join(ROOT, "openpystruct_amd", "csrc", f)).read(), f


def test_package_exports():
    import openpystruct_amd as oa
    from openpystruct_amd import frame_groups
    for name in NAMES:
        assert getattr(oa, name) is getattr(frame_groups, name) and name in oa.__all__, name
    assert frame_groups.GroupedFrameDesigns._fields == ("X", "I", "solution", "epochs", "governing", "case_penalty", "discrete")
    assert frame_groups.DiscreteDesigns._fields == ("X", "section", "I", "value", "value_continuous", "clipped")
    assert frame_groups.FrameDesignValues._fields == ("value", "case_penalty", "governing", "solution", "status")


def test_refusals_are_decided_before_any_device_call():
    """No GPU here: an entry that returns its refusal has not made a HIP call.  Every pointer is one host buffer that no refusal
    may read or write (the parameters apart: a real struct)."""
    from openpystruct_amd import _cabi, frames
    lib = _cabi.load()
    buf = ctypes.create_string_buffer(b"\xa5" * 256, 256)
    p = ctypes.addressof(buf)
    hp = frames._sizing_params(frames.FrameConfig())

    def step(G=5, C=3, Nn=4, Ne=3, Ng=2, aggregate=0, weights=None, **null):
        a = dict(geo=p, E=p, conn=p, elem_group=p, group_ptr=p, group_elems=p, X=p, I=p, I64=p, disp=p, V=p, M=p, lam=p, extra=p, st_fwd=p,
                 st_adj=p, weights=weights, aggregate=aggregate, exp_avg=p, exp_avg_sq=p, best=p, cnt=p, epochs=p, active=p, last=p,
                 penalty=p, governing=p, grad_out=p, hp=ctypes.byref(hp), schedule=p)
        a.update({k: None for k in null})
        return lib.ops_frame_group_step_f32(G, C, Nn, Ne, Ng, *a.values(), None)

    for kw in (dict(G=-1), dict(C=0), dict(C=-2), dict(Nn=1), dict(Nn=-4), dict(Ne=0, Ng=0), dict(Ne=-3), dict(Ng=0), dict(Ng=-1), dict(Ng=4),
               dict(Ne=512, Ng=513)):
        assert step(**kw) == _cabi.ERR_INVALID_ARG, kw
    assert step(Ne=513) == _cabi.ERR_UNSUPPORTED and step(C=65) == _cabi.ERR_UNSUPPORTED
    assert step(Ne=512, Ng=512, C=64, G=0) == _cabi.OK and step(G=0) == _cabi.OK and step(G=0, geo=True, elem_group=True) == _cabi.OK
    assert step(G=0, Ng=4) == _cabi.ERR_INVALID_ARG                    # the sizes are checked before G == 0 returns
    for k in ("geo", "E", "conn", "elem_group", "group_ptr", "group_elems", "X", "I", "I64", "disp", "V", "M", "lam", "exp_avg", "exp_avg_sq",
              "best", "cnt", "epochs", "active", "last", "hp"):
        assert step(**{k: True}) == _cabi.ERR_INVALID_ARG, k
    assert step(aggregate=2) == _cabi.ERR_INVALID_ARG and step(aggregate=-1) == _cabi.ERR_INVALID_ARG
    assert step(aggregate=1, weights=p) == _cabi.ERR_INVALID_ARG
    assert buf.raw == b"\xa5" * 256                                     # nothing written


def test_member_groups_checks_and_tables():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    topo = frames.grid_frame(2, 3, device="cpu")
    Ne = topo.Ne
    good = np.array([2, 0, 1] * 5)
    for bad, what in ((good[:-1], "one label per element"), (np.concatenate([good, [0]]), "one label per element"), (good.reshape(3, 5), "one label"),
                      (np.where(good == 1, -1, good), "negative"), (np.where(good == 1, 3, good), "gap"), (good + 1, "gap"),
                      (good.astype(np.float64), "integer"), (good.astype(bool), "integer"), (torch.as_tensor(good).float(), "integer")):
        with pytest.raises(ValueError, match=what):
            oa.member_groups(topo, bad)
    for labels in (good, good.astype(np.int32), good.astype(np.uint8), torch.as_tensor(good), list(good)):
        mg = oa.member_groups(topo, np.asarray(labels) if isinstance(labels, list) else labels)
        assert (mg.Ng, mg.Ne) == (3, Ne)
        assert mg.d_elem_group.dtype == mg.d_group_ptr.dtype == mg.d_group_elems.dtype == torch.int32
        assert mg.d_elem_group.tolist() == good.tolist() and mg.d_group_ptr.tolist() == [0, 5, 10, 15]
        assert mg.d_group_elems.tolist() == [1, 4, 7, 10, 13, 2, 5, 8, 11, 14, 0, 3, 6, 9, 12]      # ascending inside a group
    assert oa.member_groups(topo, mg) is mg
    with pytest.raises(ValueError, match="another topology"):
        oa.member_groups(frames.grid_frame(2, 3, device="cpu"), mg)
    X = torch.arange(6.0).reshape(2, 3)
    assert torch.equal(mg.expand(X), X[:, torch.as_tensor(good)])
    one = oa.member_groups(topo, np.zeros(Ne, dtype=np.int64))
    assert one.Ng == 1 and one.d_group_ptr.tolist() == [0, Ne] and one.d_group_elems.tolist() == list(range(Ne))


def test_story_groups():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    for bays, stories in ((1, 1), (4, 2), (2, 3)):
        topo = frames.grid_frame(bays, stories, device="cpu")
        g = oa.story_groups(topo)
        assert g.dtype == np.int32 and g.shape == (topo.Ne,) and g.max() + 1 == 2 * stories
        n_col = stories * (bays + 1)
        assert g[:n_col].max() == stories - 1 and g[n_col:].min() == stories            # columns before beams
        assert np.bincount(g).tolist() == [bays + 1] * stories + [bays] * stories
    # 2 x 3: columns 0-8 (three per story, from the ground), beams 9-14 (two per floor, from the first floor)
    assert g.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5]
    mg = oa.member_groups(topo, g)
    members = [mg.d_group_elems[mg.d_group_ptr[j]:mg.d_group_ptr[j + 1]].tolist() for j in range(mg.Ng)]
    assert members == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10], [11, 12], [13, 14]]
    y, h = topo.coords[:, 1], frames.FrameConfig().story_height
    for j, m in enumerate(members):
        for a, b in topo.conn[m]:
            assert (y[a], y[b]) == ((j * h, (j + 1) * h) if j < 3 else ((j - 2) * h, (j - 2) * h)), (j, a, b)
    # the order of the elements does not matter, only the geometry; a brace is refused
    perm = np.random.default_rng(0).permutation(topo.Ne)
    shuffled = frames.FrameTopology(topo.coords, topo.conn[perm], topo.fix3, 1.0, 1.0, 0.0, 0.0, np.zeros((topo.Nn, 3)), device="cpu")
    assert np.array_equal(oa.story_groups(shuffled), g[perm])
    flipped = frames.FrameTopology(topo.coords, topo.conn[:, ::-1], topo.fix3, 1.0, 1.0, 0.0, 0.0, np.zeros((topo.Nn, 3)), device="cpu")
    assert np.array_equal(oa.story_groups(flipped), g)
    braced = frames.FrameTopology(topo.coords, np.concatenate([topo.conn, [[0, 4]]]), topo.fix3, 1.0, 1.0, 0.0, 0.0, np.zeros((topo.Nn, 3)), device="cpu")
    with pytest.raises(ValueError, match="neither vertical nor horizontal"):
        oa.story_groups(braced)


def test_snap_to_catalogue():
    import openpystruct_amd as oa
    cat = [1.0, 2.0, 4.0, 8.0]
    #                  exact  between        tie   below  above
    X = torch.tensor([[2.0, 2.5, 3.5, 5.0, 3.0, 0.25, 9.0, 8.0, 1.5]])
    Xs, sec, clipped = oa.snap_to_catalogue(X, cat, "up")
    assert Xs.dtype == torch.float32 and sec.dtype == torch.int32 and clipped.dtype == torch.bool and Xs.shape == sec.shape == clipped.shape == X.shape
    assert Xs.tolist() == [[2.0, 4.0, 4.0, 8.0, 4.0, 1.0, 8.0, 8.0, 2.0]] and sec.tolist() == [[1, 2, 2, 3, 2, 0, 3, 3, 1]]
    assert clipped.tolist() == [[False] * 6 + [True, False, False]]
    Xn, sec, clipped = oa.snap_to_catalogue(X, cat, "nearest")
    assert Xn.tolist() == [[2.0, 2.0, 4.0, 4.0, 4.0, 1.0, 8.0, 8.0, 2.0]] and sec.tolist() == [[1, 1, 2, 2, 2, 0, 3, 3, 1]]      # ties (3.0, 1.5) go up
    assert clipped.tolist() == [[False] * 6 + [True, False, False]]
    assert oa.snap_to_catalogue(X, cat)[0].tolist() == Xs.tolist()                  # "up" is the default
    assert oa.snap_to_catalogue(X.double(), np.array(cat), "up")[0].dtype == torch.float32
    one = oa.snap_to_catalogue(torch.tensor([0.5, 3.0, 7.0]), [3.0], "nearest")
    assert one[0].tolist() == [3.0, 3.0, 3.0] and one[1].tolist() == [0, 0, 0] and one[2].tolist() == [False, False, True]
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, 1.0], [-1.0, 1.0], [1.0, float("nan")], [1.0, float("inf")], [1.0, 1.0 + 1e-12]):
        with pytest.raises(ValueError, match="catalogue"):
            oa.snap_to_catalogue(X, bad)
    with pytest.raises(ValueError, match="mode"):
        oa.snap_to_catalogue(X, cat, "down")
    with pytest.raises(ValueError, match="floating"):
        oa.snap_to_catalogue(torch.tensor([1, 2]), cat)


def test_python_entries_check_groups_and_shapes_then_devices():
    import openpystruct_amd as oa
    from openpystruct_amd import frames
    topo = frames.grid_frame(1, 1, device="cpu")
    G, C = 2, 3
    f64 = dict(dtype=torch.float64)
    loads, w = torch.zeros((G, C, topo.Nn, 3), **f64), torch.zeros((G, C, topo.Ne, 2), **f64)
    groups = oa.story_groups(topo)
    X0 = torch.full((G, 2), 5e-4)
    for bad in (groups[:-1], groups + 1, -groups, groups.astype(np.float32)):
        with pytest.raises(ValueError, match="groups"):
            oa.optimize_grouped_frame_designs(topo, bad, loads)
    for bad in (loads[..., :2], loads.float(), loads[0, 0]):
        with pytest.raises(ValueError, match="loads must be"):
            oa.optimize_grouped_frame_designs(topo, groups, bad, n_designs=G)
    with pytest.raises(ValueError, match="n_designs or X0"):
        oa.optimize_grouped_frame_designs(topo, groups, loads[0])
    with pytest.raises(ValueError, match="X0 must be"):
        oa.optimize_grouped_frame_designs(topo, groups, loads, X0=torch.full((G, topo.Ne), 5e-4))
    with pytest.raises(ValueError, match="element_loads"):
        oa.optimize_grouped_frame_designs(topo, groups, loads, w[:, :2])
    for kw in (dict(weights=(1.0, 1.0)), dict(aggregate="max", weights=(1.0, 1.0, 1.0)), dict(aggregate="mean"), dict(alpha_sway=1.0),
               dict(snap="down"), dict(catalogue=[2.0, 1.0]), dict(catalogue=[])):
        with pytest.raises(ValueError):
            oa.optimize_grouped_frame_designs(topo, groups, loads, **kw)
    big = frames.grid_frame(16, 16, device="cpu", numbering="node")
    with pytest.raises(ValueError, match="512"):
        oa.optimize_grouped_frame_designs(big, oa.story_groups(big), torch.zeros((1, 2, big.Nn, 3), **f64))
    for args, kw in (((loads,), {}), ((loads, w), {}), ((loads,), dict(X0=X0, aggregate="max", catalogue=[1e-4, 1e-3]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            oa.optimize_grouped_frame_designs(topo, groups, *args, **kw)
    # evaluate_frame_designs
    I = torch.full((G, topo.Ne), 5e-4)
    for bad in (I[:, :-1], I.to(torch.int32), I[0], I.numpy()):
        with pytest.raises(ValueError, match="I must be"):
            oa.evaluate_frame_designs(topo, bad, loads)
    with pytest.raises(ValueError, match="I must be"):
        oa.evaluate_frame_designs(topo, I[:1], loads)
    with pytest.raises(ValueError):
        oa.evaluate_frame_designs(topo, I, loads, alpha_deflection=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.evaluate_frame_designs(topo, I, loads, w)
    # frame_group_gradient: the checks of frame_design_gradient, the groups first
    I64 = I.double()
    sol0 = frames.FrameSolution(torch.zeros((G, topo.Nn, 3), **f64), torch.zeros((G, topo.Ne, 6), **f64), torch.zeros((G, topo.Ne), **f64),
                                torch.zeros((G, topo.Ne), **f64), torch.zeros((G,), dtype=torch.int32))
    fac = frames.FrameFactor(topo, I64, torch.zeros(16, dtype=torch.uint8), sol0)
    case = frames.FrameCaseSolution(torch.zeros((G, C, topo.Nn, 3), **f64), torch.zeros((G, C, topo.Ne, 6), **f64),
                                    torch.zeros((G, C, topo.Ne), **f64), torch.zeros((G, C, topo.Ne), **f64), torch.zeros((G, C), dtype=torch.int32))
    cfg = frames.FrameConfig()
    with pytest.raises(ValueError, match="groups"):
        oa.frame_group_gradient(fac, case, groups + 1, cfg)
    with pytest.raises(ValueError, match="sol\\."):
        oa.frame_group_gradient(fac, case._replace(V=case.V.float()), groups, cfg)
    with pytest.raises(ValueError):
        oa.frame_group_gradient(fac, case, groups, cfg, aggregate="max", weights=(1.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        oa.frame_group_gradient(fac, case, groups, cfg)
    with pytest.raises(ValueError, match="story"):
        oa.generate_grouped_frame_design_dataset(1, 1, 2, 2, groups="floor")


@pytest.mark.parametrize("frame", ["2x3", "4x2"])
def test_segment_sum_of_the_design_gradient_is_autograd_with_one_leaf_per_group(frame):
    """The chain rule on the dense float64 model: both sides are float64 sums of the same terms -- 1e-12 relative."""
    from openpystruct_amd import frames
    from tests import frame_dense as fd
    from tests import frame_designs_ref as dr
    from tests import frame_groups_ref as gr
    from tests import frame_sizing_total_ref as ft
    bays, stories = (int(v) for v in frame.split("x"))
    topo = frames.grid_frame(bays, stories, device="cpu")
    case = fd.case_of(topo)
    G, C = 3, 3
    rng = np.random.default_rng(41 + bays)
    H, q = rng.uniform(0.5e4, 2e4, size=G), rng.uniform(-2e4, -0.5e4, size=G)
    loads, w = frames.grid_load_cases(topo, np.stack([H, -H, 0 * H], 1).reshape(-1), np.stack([q, q, 1.5 * q], 1).reshape(-1))
    loads, w = loads.numpy().reshape(G, C, topo.Nn, 3), w.numpy().reshape(G, C, topo.Ne, 2)
    hp = ft.frame_hp()
    for kind in ("story", "random"):
        labels = gr.group_table(topo, kind)
        Ng = labels.max() + 1
        X = fd.random_inertias(rng, G, topo.Ne)[:, :Ng]
        I = X[:, labels]
        free = dr.design_gradient(case, I, loads, w, hp, ft.objective(), dr.SUM)
        assert np.array_equal(gr.segment_sum(np.ones((G, topo.Ne)), labels), np.tile(np.bincount(labels).astype(np.float64), (G, 1)))
        for obj in (ft.objective(), ft.objective(3.0, 5e-4, 2.0, 4e-4)):
            for aggregate, weights in ((dr.SUM, None), (dr.SUM, (1.0, 1.0, 0.5)), (dr.MAX, None)):
                per_elem = dr.design_gradient(case, I, loads, w, hp, obj, aggregate, weights)
                want = gr.group_gradient(case, X, labels, loads, w, hp, obj, aggregate, weights)
                got = gr.segment_sum(per_elem.grad, labels)
                err = float(np.abs(got - want.grad).max() / np.abs(want.grad).max())
                print(f"{frame} {kind} aggregate {aggregate} weights {weights} hinges {obj.alpha_sway > 0}: {err:.3e}")
                assert err <= 1e-12, (kind, aggregate, weights, err)
                assert np.array_equal(per_elem.governing, want.governing) and np.allclose(per_elem.loss, want.loss, rtol=1e-14)
        assert free.grad.shape == (G, topo.Ne)
