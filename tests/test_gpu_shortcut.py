"""Path shortcutting on the device: the connect table of all pairs of a path
(k_shortcut_pairs, gbp_shortcut_table_dev) against the oracle's attemptConnect
decisions, and postProcessPath over it (gbp_shortcut_paths_host,
planner.shortcut_paths, post_process=2) against orc_post_process_path
(rrt_connect.cpp:139-227), bit for bit.
"""
import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import engine, planner
from tests import shortcut_cases as C
from tests.helpers import bits

pytestmark = pytest.mark.gpu

_terrains = {}


def _terrain(name, fragile_eps=None):
    """One engine Terrain per (terrain, FRAGILE margin) for the module."""
    key = (name, fragile_eps)
    if key not in _terrains:
        T = engine.Terrain.from_data(C.terrain(name)[0], device=0)
        if fragile_eps is not None:
            T.set_option(L.OPT_FRAGILE_EPS, int(round(fragile_eps * 1e15)))
        _terrains[key] = T
    return _terrains[key]


_tables = {}


def _oracle_table(case, batch, seed, k, adaptive):
    key = (case, batch, seed, k, adaptive)
    if key not in _tables:
        S, _ = C.dense_path(case, batch, seed, k)
        _tables[key] = C.oracle_table(case[0], S, adaptive)
    return _tables[key]


def _resolved_table(T, name, states, adaptive):
    """The device table with its FRAGILE items re-decided the way
    gbp_shortcut_paths_host does: through that entry on the two-state path of
    each flagged pair (REACHED there keeps the connect action, a[7] = 0; the
    fallback keeps the marker action)."""
    reached, flags = T.shortcut_table([states], adaptive=adaptive)
    reached = reached.cpu().numpy().copy()
    flags = flags.cpu().numpy().view(np.uint32)
    assert set(np.unique(reached)) <= {0, 1}
    assert not np.any(flags & ~np.uint32(L.F_OOD | L.F_NAN | L.F_FRAGILE | L.F_LIMIT))
    pr = C.pairs(len(states))
    frag = np.flatnonzero(flags & L.F_FRAGILE)
    if frag.size:
        marker = np.zeros((1, 10))
        marker[0, 6], marker[0, 7] = 0.1, 1.0
        out = planner.shortcut_paths(T, [states[list(pr[it])] for it in frag],
                                     [marker] * frag.size, adaptive=adaptive)
        assert out["n_resolved"] == frag.size
        for it, a in zip(frag, out["actions"]):
            reached[it] = 1 if a[0, 7] == 0 else 0
    return reached, int(frag.size)


@pytest.mark.parametrize("grid", [None, 2])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case,batch,seed,k,n_states", [d + (n,) for d, n in zip(C.DENSE, (106, 109))])
def test_table_equals_oracle(gpu, monkeypatch, case, batch, seed, k, n_states, adaptive, grid):
    """Every pair of the densified found path; with a grid of 2 workgroups each
    wave takes hundreds of pairs."""
    if grid is not None:
        monkeypatch.setenv("GBP_SHORTCUT_GRID", str(grid))
    S, _ = C.dense_path(case, batch, seed, k)
    assert len(S) == n_states
    want = _oracle_table(case, batch, seed, k, adaptive)
    share = want.mean()
    print(f"{case[0]} adaptive {adaptive}: {want.size} pairs, {100 * share:.1f} % REACHED")
    assert 0.05 <= share <= 0.95  # neither outcome goes untested
    got, nres = _resolved_table(_terrain(case[0]), case[0], S, adaptive)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:10], [C.pairs(len(S))[b] for b in bad[:10]], nres)


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case,batch,seed,k", C.DENSE)
def test_table_forced_fragile(gpu, case, batch, seed, k, adaptive):
    """The FRAGILE margin widened to 1e-5 (as test_gpu_oracle_loop.py does):
    pairs are flagged, re-decided on the host, and the table is the same."""
    S, _ = C.dense_path(case, batch, seed, k)
    want = _oracle_table(case, batch, seed, k, adaptive)
    got, nres = _resolved_table(_terrain(case[0], 1e-5), case[0], S, adaptive)
    print(f"{case[0]} adaptive {adaptive}: {nres} of {want.size} pairs re-decided")
    assert nres > 0
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("order", [0, 1])
def test_table_item_order_gives_the_same_table(gpu, monkeypatch, order):
    """The kernel's two item orders (a path's pairs as packed / longest spans
    first) write the same table; three paths in one launch, a grid of 3."""
    monkeypatch.setenv("GBP_SHORTCUT_ORDER", str(order))
    T = _terrain(C.SYNTH[0])
    paths = [C.found_path(C.SYNTH, 64, 5)[0], C.found_path(C.SYNTH, 64, 11)[0][:2],
             C.found_path(C.SYNTH, 64, 3)[0]]
    want = np.concatenate([C.oracle_table(C.SYNTH[0], p, False) for p in paths])
    for grid in (None, 3):
        if grid is not None:
            monkeypatch.setenv("GBP_SHORTCUT_GRID", str(grid))
        reached, flags = T.shortcut_table(paths)
        keep = (flags.cpu().numpy().view(np.uint32) & L.F_FRAGILE) == 0
        assert np.array_equal(reached.cpu().numpy()[keep], want[keep])


def _assert_paths_equal(out, p, want, label):
    ws, wa, wl, wy, wc = want
    assert out["states"][p].shape == ws.shape, (label, out["states"][p].shape, ws.shape)
    assert np.array_equal(bits(out["states"][p]), bits(ws)), (label, "states")
    assert np.array_equal(bits(out["actions"][p]), bits(wa)), (label, "actions")
    assert bits(out["path_length"][p]) == bits(wl), (label, "path_length_")
    assert bits(out["path_yaw"][p]) == bits(wy), (label, "path_yaw_")
    assert bits(out["path_cost"][p]) == bits(wc), (label, "path_cost_")


@pytest.mark.parametrize("fragile_eps", [None, 1e-5])
@pytest.mark.parametrize("adaptive", [False, True])
def test_shortcut_paths_equal_oracle(gpu, adaptive, fragile_eps):
    """planner.shortcut_paths on the found paths, each terrain's in one call;
    with the FRAGILE margin widened to 1e-5 pairs are re-decided on the host and
    nothing changes."""
    resolved = 0
    for terr in (C.SYNTH, C.SLOPE):
        cases = [c for c in C.FOUND if c[0] is terr]
        paths = [C.found_path(*c, adaptive) for c in cases]
        out = planner.shortcut_paths(_terrain(terr[0], fragile_eps), [p[0] for p in paths],
                                     [p[1] for p in paths], adaptive=adaptive)
        for p, (c, (S, A)) in enumerate(zip(cases, paths)):
            _assert_paths_equal(out, p, C.oracle_walk(terr[0], S, A, adaptive), (c, adaptive))
        resolved += out["n_resolved"]
    print(f"adaptive {adaptive} fragile_eps {fragile_eps}: {resolved} pairs re-decided")
    if fragile_eps is not None:
        assert resolved > 0


@pytest.mark.parametrize("fragile_eps", [None, 1e-5])
@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("case,batch,seed,k,after,fallback", [
    C.DENSE[0] + ((3, 2), (0, 0)), C.DENSE[1] + ((9, 10), (0, 1))])
def test_dense_paths_batched(gpu, case, batch, seed, k, after, fallback, adaptive, fragile_eps):
    """Three paths of different lengths in one call — the densified path, the
    two-state path of its ends' first edge, a found path — give each path's
    single-call result, and the densified one the oracle's walk."""
    T = _terrain(case[0], fragile_eps)
    S, A = C.dense_path(case, batch, seed, k)
    fs, fa = C.found_path(case, batch, seed, adaptive)
    paths, acts = [S, fs[:2], fs], [A, fa[:1], fa]
    want = C.oracle_walk(case[0], S, A, adaptive)
    assert len(want[0]) == after[int(adaptive)]
    assert C.fallback_edges(want[1]) == fallback[int(adaptive)]
    out = planner.shortcut_paths(T, paths, acts, adaptive=adaptive)
    _assert_paths_equal(out, 0, want, "dense")
    _assert_paths_equal(out, 1, C.oracle_walk(case[0], fs[:2], fa[:1], adaptive), "two states")
    _assert_paths_equal(out, 2, C.oracle_walk(case[0], fs, fa, adaptive), "found")
    for p in range(3):
        one = planner.shortcut_paths(T, paths[p:p + 1], acts[p:p + 1], adaptive=adaptive)
        for key in ("states", "actions"):
            assert np.array_equal(bits(one[key][0]), bits(out[key][p])), (p, key)
        for key in ("path_length", "path_yaw", "path_cost"):
            assert bits(one[key][0]) == bits(out[key][p]), (p, key)
    if fragile_eps is not None:
        assert out["n_resolved"] > 0


@pytest.mark.parametrize("fragile_eps", [None, 1e-5])
@pytest.mark.parametrize("algorithm", [3, 0])
@pytest.mark.parametrize("case,batch,seed", [(C.SYNTH, 64, 11), (C.SLOPE, 256, 7)])
def test_post_process_device_equals_host(gpu, algorithm, case, batch, seed, fragile_eps):
    """plan_rrt_connect(post_process=2) against post_process=True, field for
    field (the search is the same; only postProcessPath's form differs)."""
    data, O = C.terrain(case[0])
    start, goal = C.start_goal(O, *case[1])
    kw = dict(batch=batch, max_time=300.0, seed=seed, algorithm=algorithm, fragile_eps=fragile_eps)
    host = planner.plan_rrt_connect(data, start, goal, post_process=True, **kw)
    dev = planner.plan_rrt_connect(data, start, goal, post_process=2, **kw)
    assert host["found"] == 1
    timing = {"time_to_first", "total_time", "stage_us", "stage_halves"}
    for key in host:
        if key in timing:
            continue
        if isinstance(host[key], np.ndarray):
            assert np.array_equal(bits(host[key]), bits(dev[key])), key
        else:
            assert host[key] == dev[key], key
    want = C.oracle_walk(case[0], *C.found_path(case, batch, seed), False)
    assert np.array_equal(bits(dev["states"]), bits(want[0]))
    assert np.array_equal(bits(dev["actions"]), bits(want[1]))


# ---- more paths in a call than a launch takes ------------------------------------------------
def _window_tables(T, paths, adaptive):
    """The device table of a call of many paths, split per path, its FRAGILE
    items re-decided as _resolved_table re-decides them."""
    reached, flags = T.shortcut_table(paths, adaptive=adaptive)
    reached = reached.cpu().numpy().copy()
    flags = flags.cpu().numpy().view(np.uint32)
    assert set(np.unique(reached)) <= {0, 1}
    assert not np.any(flags & ~np.uint32(L.F_OOD | L.F_NAN | L.F_FRAGILE | L.F_LIMIT))
    sizes = [len(p) * (len(p) - 1) // 2 for p in paths]
    assert reached.size == sum(sizes)
    off = np.r_[0, np.cumsum(sizes)]
    frag = np.flatnonzero(flags & L.F_FRAGILE)
    if frag.size:
        marker = np.zeros((1, 10))
        marker[0, 6], marker[0, 7] = 0.1, 1.0
        two = []
        for it in frag:
            p = int(np.searchsorted(off, it, side="right")) - 1
            two.append(paths[p][list(C.pairs(len(paths[p]))[it - off[p]])])
        out = planner.shortcut_paths(T, two, [marker] * frag.size, adaptive=adaptive)
        assert out["n_resolved"] == frag.size
        for it, a in zip(frag, out["actions"]):
            reached[it] = 1 if a[0, 7] == 0 else 0
    return [reached[off[p]:off[p + 1]] for p in range(len(paths))], int(frag.size)


_singles = {}


def _window_reference(dense, adaptive, T):
    """Per window: (the dense table's sub-block, the oracle's walk, the
    window's single-path call), once per (path, adaptive)."""
    key = (dense, adaptive)
    if key not in _singles:
        from tests import scale_cases as X
        case = C.DENSE[dense]
        n = len(C.dense_path(*case)[0])
        table = _oracle_table(*case, adaptive)
        paths, acts = X.window_paths(dense)
        blocks = [X.window_block(table, n, o, m) for o, m in X.windows(dense)]
        walks = [C.oracle_walk(case[0][0], S, A, adaptive) for S, A in zip(paths, acts)]
        ones = [planner.shortcut_paths(T, [S], [A], adaptive=adaptive) for S, A in zip(paths, acts)]
        _singles[key] = (paths, acts, blocks, walks, ones)
    return _singles[key]


@pytest.mark.parametrize("dense,adaptive,grid", [(0, False, None), (0, True, None), (1, False, None),
                                                 (1, True, None), (0, False, 2)])
def test_more_paths_than_a_launch_takes(gpu, monkeypatch, dense, adaptive, grid):
    """65, 128 and 150 windows of a densified path in one call: two and three
    launches of up to 64 paths, the later ones carrying the first item and the
    absolute path and pair offsets of their group.  Every window's table is the
    dense path's sub-block, its walk the oracle's and its single-path call's."""
    if grid is not None:     # two workgroups: every wave takes many items of every launch
        monkeypatch.setenv("GBP_SHORTCUT_GRID", str(grid))
    from tests import scale_cases as X
    T = _terrain(C.DENSE[dense][0][0])
    paths, acts, blocks, walks, ones = _window_reference(dense, adaptive, T)
    reached_share = np.concatenate(blocks).mean()
    assert 0.05 <= reached_share <= 0.95
    for count in X.WINDOW_CALLS:
        tables, nres = _window_tables(T, paths[:count], adaptive)
        for p in range(count):
            assert np.array_equal(tables[p], blocks[p]), (count, p, X.windows(dense)[p], nres)
        out = planner.shortcut_paths(T, paths[:count], acts[:count], adaptive=adaptive)
        for p in range(count):
            _assert_paths_equal(out, p, walks[p], (count, p))
            for key in ("states", "actions"):
                assert np.array_equal(bits(ones[p][key][0]), bits(out[key][p])), (count, p, key)
            for key in ("path_length", "path_yaw", "path_cost"):
                assert bits(ones[p][key][0]) == bits(out[key][p]), (count, p, key)
