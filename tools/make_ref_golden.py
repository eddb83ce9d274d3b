"""Generate tests/golden/reference_vectors.npz from the COMPILED REFERENCE.

    python -c "import __graft_entry__ as g; g.build()"   # builds oracle/_ref/libgbp_ref.so
    python tools/make_ref_golden.py

Runs on the CPU against oracle/_ref/libgbp_ref.so: the reference planner's own
seven ROS-free sources, unmodified, plus oracle/ref/ref_driver.cpp, compiled
with three stand-in headers (oracle/ref/stubs).  The fixture holds data only
(plain arrays, no pickle): selections into the inputs of tests/ref_cases.py and
the reference's recorded outputs for them.

What this pins: FastTerrainMap's lookups behind loadData, planning_utils'
closed forms and getInterpPath, isValidState, the four pair checks, both attemptConnect
overloads, PlannerClass / GraphClass trees (neighbour searches, g / y, paths,
the join), RRTConnectClass::connect and postProcessPath, and RRT / RRT* extend
by record and replay (the drawn action of each insertion is recorded as data).
What it does not: grid_map's CSV -> geometry path, Eigen proper (keys under
"eigen/" are "reference + stand-in Eigen": rotate_grf is the only function
that touches it), the samplers (rand() and clock-seeded engines against
Philox), the full search loop, and nearest-neighbour ties.

Cases outside the reference's defined domain (tests/ref_cases.py) are screened
out with the oracle's flags and never passed to the reference; the screened
share per entry is printed and stored under "screened/", and must stay within
ref_cases.CAPS.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from oracle import reflib  # noqa: E402
from tests import ref_cases as C  # noqa: E402

# keys that record what the reference drew (rand() / clock-seeded): inputs of
# the replays, not reproducible from one run to the next
DRAWN_PREFIX = "replay/"


def _bits_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return a != b


def _terrain_entries(name, out, screened):
    data, O = C.terrain(name)
    R = reflib.RefTerrain.from_data(data)
    b = C.base_inputs(name)
    p = name + "/"
    # lookups
    bad = C.lookup_screen(name)
    keep = np.flatnonzero(~bad)
    h, nan, nrm = R.lookups(b["xy"][keep])
    out.update({p + "lk_keep": keep.astype(np.int32), p + "lk_h": h, p + "lk_nan": nan,
                p + "lk_normal": nrm})
    screened["lookups"].append((name, int(bad.sum()), bad.size))
    # isValidState
    for ph in (0, 1):
        bad = C.state_screen(name, ph)
        keep = np.flatnonzero(~bad)
        out[p + f"vs_keep_{ph}"] = keep.astype(np.int32)
        out[p + f"vs_valid_{ph}"] = R.valid_states(b["states"][keep], ph)
        screened["valid_states"].append((name, int(bad.sum()), bad.size))
    # pair checks, each row in its own direction (the rows alternate)
    for ad in (0, 1):
        bad = C.pair_screen(name, ad)
        keep = np.flatnonzero(~bad)
        v, sn, tn = R.pairs(b["pair_s"][keep], b["pair_a"][keep], b["pair_dir"][keep], ad,
                            C.S_UNSET, C.T_UNSET)
        out.update({p + f"pr_keep_{ad}": keep.astype(np.int32), p + f"pr_valid_{ad}": v,
                    p + f"pr_s_new_{ad}": sn, p + f"pr_t_new_{ad}": tn})
        screened["pairs"].append((name, int(bad.sum()), bad.size))
    # connects, two-state overload: row k direction k & 1, adaptive (k >> 1) & 1
    e_idx, s_idx = C.connect_candidates(name)
    pool = b["pool"]
    k = np.arange(e_idx.size)
    bad = np.array([C.connect_undefined(O, pool[e], pool[s], int(i & 1), int((i >> 1) & 1))
                    for i, e, s in zip(k, e_idx, s_idx)])
    keep = np.flatnonzero(~bad)
    res = np.empty(keep.size, np.int32)
    sn, an = np.empty((keep.size, 8)), np.empty((keep.size, 10))
    for ad in (0, 1):
        m = ((keep >> 1) & 1) == ad
        r, s1, a1 = R.connects(pool[e_idx[keep[m]]], pool[s_idx[keep[m]]], keep[m] & 1, ad)
        res[m], sn[m], an[m] = r, s1, a1
    out.update({p + "cn_e": e_idx.astype(np.int32), p + "cn_s": s_idx.astype(np.int32),
                p + "cn_keep": keep.astype(np.int32), p + "cn_result": res, p + "cn_s_new": sn,
                p + "cn_a_new": an})
    screened["connects"].append((name, int(bad.sum()), bad.size))
    # connects, t_s overload: the nearest-state pairs with t_s around KINEMATICS_RES
    ts = C.ts_cases()
    near = np.flatnonzero(k % 2 == 1)[:ts.size * 2]
    tsv = np.tile(ts, 2)[:near.size]
    bad = np.array([C.connect_undefined(O, pool[e_idx[i]], pool[s_idx[i]], int(i & 1),
                                        int((i >> 1) & 1), t_s=t) for i, t in zip(near, tsv)])
    rows, tsk = near[~bad], tsv[~bad]
    res = np.empty(rows.size, np.int32)
    sn, an = np.empty((rows.size, 8)), np.empty((rows.size, 10))
    for ad in (0, 1):
        m = ((rows >> 1) & 1) == ad
        if m.any():
            res[m], sn[m], an[m] = R.connects(pool[e_idx[rows[m]]], pool[s_idx[rows[m]]],
                                              rows[m] & 1, ad, t_s=tsk[m])
    out.update({p + "ct_row": rows.astype(np.int32), p + "ct_ts": tsk, p + "ct_result": res,
                p + "ct_s_new": sn, p + "ct_a_new": an})
    screened["connects"].append((name + " (t_s)", int(bad.sum()), bad.size))
    return R


def _forms(out):
    s, s2, a, t = C.form_inputs()
    out["cf/apply"] = reflib.apply(s, a, t)
    d, w = reflib.distances(s, s2, *C.YAW_WEIGHTS)
    out["cf/dist"], out["cf/within"] = d, w
    out["cf/valid_action"] = reflib.valid_actions(a)
    out["cf/interp"] = reflib.interp(s, s2, t)
    # reference + stand-in Eigen: surface normals of the golden lookups, forces
    # from the golden actions (mass * acceleration)
    nrm = C.oracle_vectors()[C.TREE_TERRAIN + "/normal"][:C.N_FORMS]
    ok = np.isfinite(nrm).all(axis=1)
    nrm = np.where(ok[:, None], nrm, [0.0, 0.0, 1.0])
    out["eigen/rotate_grf"] = reflib.rotate_grf(nrm, 13.0 * (a[:, :3] + [0, 0, 9.81]))
    out["eigen/normals"] = nrm


def _trees(out, R):
    verts, parent, act, queries = C.tree_vertices()
    assert C.no_exact_ties(verts, queries), "the neighbour-search queries must see no exact ties"
    for n in C.TREE_SIZES:
        for yaw in (None, C.YAW_WEIGHTS):
            t = reflib.RefTree(verts[0], yaw=yaw)
            for i in range(1, n):
                t.add(i, verts[i], parent[i], act[i])
            p = f"nbr/{n}/"
            if yaw is None:
                out[p + "nearest"] = t.nearest(queries)
                lists = [t.neighborhood_dist(q, C.NBR_RADIUS) for q in queries]
                out[p + "dist_cnt"] = np.array([len(x) for x in lists], np.int32)
                out[p + "dist_idx"] = np.concatenate(lists).astype(np.int32)
                out[p + "knn"] = np.array([t.neighborhood_n(q, C.KNN_K) for q in queries], np.int32)
                if n == max(C.TREE_SIZES):
                    d = t.dump()
                    assert np.array_equal(d["parent"], parent[:n])
                    out["tree/g"], out["tree/y"] = d["g"], d["y"]
                    for j, idx in enumerate([0, 1, 7, 100, 256, 257, 599]):
                        pa, st, ac, ar = t.path(idx)
                        out[f"tree/path{idx}"] = pa
                        out[f"tree/path{idx}_states"], out[f"tree/path{idx}_actions"] = st, ac
                        out[f"tree/path{idx}_actions_rev"] = ar
                    # updateGYValue: a new g / y at vertex 1 propagates down its subtree
                    t.update_gy(1, 10.0, 0.25)
                    d2 = t.dump()
                    out["tree/g_after_update"], out["tree/y_after_update"] = d2["g"], d2["y"]
            else:
                out[p + "knn_yaw"] = np.array([t.neighborhood_n(q, C.KNN_K) for q in queries], np.int32)
    # the join of two half paths: Ta the first 257 vertices, Tb the next 300
    ta, tb = reflib.RefTree(verts[0]), reflib.RefTree(verts[257])
    for i in range(1, 257):
        ta.add(i, verts[i], parent[i], act[i])
    for i in range(1, 300):
        tb.add(i, verts[257 + i], parent[i], act[257 + i])
    for ia, ib in [(256, 299), (0, 0), (5, 0), (0, 17), (123, 45)]:
        st, ac = reflib.join(ta, tb, ia, ib)
        out[f"join/{ia}_{ib}_states"], out[f"join/{ia}_{ib}_actions"] = st, ac
    # the graft check's connects: attemptConnect(root, vertex) for every vertex
    graft_screened = []
    for direction, adaptive in C.ROOT_CONNECT_CONFIGS:
        bad = C.graft_screen(direction, adaptive)
        keep = np.flatnonzero(~bad)
        g_root, g_verts = C.graft_vertices()
        r, _, an = R.connects(np.broadcast_to(g_root, (keep.size, 8)), g_verts[keep], direction,
                              adaptive)
        p = f"graft/{direction}{adaptive}/"
        out[p + "keep"], out[p + "result"] = keep.astype(np.int32), r.astype(np.int8)
        out[p + "actions"] = an[r == oracle.REACHED]
        graft_screened.append((f"graft {direction}{adaptive}", int(bad.sum()), bad.size))
    # RRTConnectClass::connect toward 24 far states, the tree growing as it goes
    _, O = C.terrain(C.TREE_TERRAIN)
    t = reflib.RefTree(verts[0])
    for i in range(1, 128):
        t.add(i, verts[i], parent[i], act[i])
    targets = verts[300:324]
    nn, rc, rows, skipped = [], [], [], 0
    for k, s in enumerate(targets):
        direction, adaptive = k & 1, (k >> 1) & 1
        d = t.dump()
        near = int(t.nearest(s)[0])
        if C.connect_undefined(O, d["v"][near], s, direction, adaptive):
            skipped += 1
            nn.append(-1), rc.append(-1)
            continue
        r = t.connect(R, s, direction, adaptive)
        nn.append(near), rc.append(r)
        if r != oracle.TRAPPED:
            d = t.dump()
            rows.append(np.concatenate([d["v"][-1], d["act"][-1], [d["parent"][-1], d["g"][-1],
                                                                   d["y"][-1]]]))
    out["tconn/nearest"], out["tconn/result"] = np.array(nn, np.int32), np.array(rc, np.int32)
    out["tconn/rows"] = np.array(rows).reshape(-1, 21)
    return [("tree connect", skipped, len(targets))] + graft_screened


def _post_process(out, terrains):
    total = bad = 0
    for key, name, S, A, adaptive in C.path_cases():
        _, O = C.terrain(name)
        oracle.set_scan_mode(1)
        total += 1
        if any(C.connect_undefined(O, S[i], S[j], oracle.FORWARD, adaptive)
               for i in range(len(S)) for j in range(i + 1, len(S))):
            bad += 1
            oracle.set_scan_mode(0)
            continue
        oracle.set_scan_mode(0)
        R = terrains[name]
        st, ac, fig = R.post_process(S, A, adaptive)
        st2, ac2, figy = R.post_process(S, A, adaptive, yaw=C.YAW_WEIGHTS)
        assert not _bits_differ(st, st2).any() and not _bits_differ(ac, ac2).any()
        p = "pp/" + key + "/"
        out.update({p + "states": st, p + "actions": ac, p + "fig": fig, p + "fig_yaw": figy})
        # the all-pairs connect table (row-major upper triangle); the REACHED
        # pairs' actions for the found paths only (at most ~40 states)
        ii, jj = np.triu_indices(len(S), 1)
        r, _, an = R.connects(S[ii], S[jj], 0, adaptive)
        out[p + "table"] = r.astype(np.int8)
        if len(S) <= 40:
            out[p + "table_actions"] = an[r == oracle.REACHED]
    return bad, total


def _interp_paths(out):
    """getInterpPath on a few paths: points, times and phases."""
    for key, S, A, dt in C.interp_path_cases(out):
        path, t, phase = reflib.interp_path(S, A, dt)
        p = "ip/" + key + "/"
        out.update({p + "path": path, p + "t": t, p + "phase": phase})


def _replays(out, R):
    """Record RRT / RRT* extend: after srand(fixed) the real extend runs toward
    each target; the nearest vertex queried just before, the return code and the
    whole tree after each call are kept (as the rows that changed)."""
    verts = C.replay_vertices()
    _, O = C.terrain(C.TREE_TERRAIN)
    bad = total = 0
    for key, direction, adaptive, star, n0, stream in C.replay_trees():
        targets = C.replay_targets(stream)
        reflib.srand(20251021)
        parent = C.replay_parents(n0)
        t = reflib.RefTree(verts[0])
        for i in range(1, n0):
            t.add(i, verts[i], parent[i], np.zeros(10))
        prev = t.dump()
        p = DRAWN_PREFIX + key + "/"
        out[p + "parent0"], out[p + "g0"], out[p + "y0"] = parent, prev["g"], prev["y"]
        nn, rc, tgs, step, idx, rows, defined = [], [], [], [], [], [], []
        inserted = 0
        for j, tg in enumerate(targets):
            if inserted == C.REPLAY_INSERTIONS:
                break
            near = int(t.nearest(tg)[0])
            r = t.extend(R, tg, direction, adaptive, star)
            if r == oracle.TRAPPED:
                assert t.n == prev["parent"].size
                continue
            nn.append(near), rc.append(r), tgs.append(tg)
            j = inserted
            inserted += 1
            cur = t.dump()
            n_prev = prev["parent"].size
            for i in range(cur["parent"].size):
                row = np.concatenate([cur["v"][i], cur["act"][i], [cur["parent"][i], cur["g"][i],
                                                                   cur["y"][i]]])
                if i >= n_prev:
                    changed = True
                else:
                    old = np.concatenate([prev["v"][i], prev["act"][i],
                                          [prev["parent"][i], prev["g"][i], prev["y"][i]]])
                    changed = _bits_differ(row, old).any()
                if changed:
                    step.append(j), idx.append(i), rows.append(row)
            total += 1
            ok = True
            if star:
                new = cur["v"][-1]
                nb, cnt = oracle.neighbors_batch(new[None], prev["v"], C.STAR_DELTA,
                                                 max_out=prev["parent"].size)
                ok = not any(C.connect_undefined(O, prev["v"][i], new, direction, adaptive) or
                             C.connect_undefined(O, new, prev["v"][i], direction, adaptive)
                             for i in nb[0, :cnt[0]])
            bad += not ok
            defined.append(ok)
            prev = cur
        assert inserted == C.REPLAY_INSERTIONS, (key, inserted)
        out.update({p + "nearest": np.array(nn, np.int32), p + "result": np.array(rc, np.int32),
                    p + "targets": np.array(tgs), p + "defined": np.array(defined, np.uint8),
                    p + "chg_step": np.array(step, np.int32), p + "chg_idx": np.array(idx, np.int32),
                    p + "chg_rows": np.array(rows).reshape(-1, 21)})
    return bad, total


def generate(verbose=True, replays=True):
    """All arrays of the fixture, from the compiled reference (replays=False:
    without the record-and-replay entries, whose draws differ run by run)."""
    oracle.set_scan_mode(0)
    out = {}
    screened = {k: [] for k in C.CAPS}
    terrains = {name: _terrain_entries(name, out, screened) for name in C.TERRAINS}
    _forms(out)
    screened["connects"] += _trees(out, terrains[C.TREE_TERRAIN])
    b, n = _post_process(out, terrains)
    screened["post_process"].append(("paths", b, n))
    _interp_paths(out)
    if replays:
        b, n = _replays(out, terrains[C.TREE_TERRAIN])
        screened["replays"].append(("insertions", b, n))
    for entry, rows in screened.items():
        for label, b, n in rows:
            share = b / max(n, 1)
            if verbose:
                print(f"screened {entry:13s} {label:32s} {b:4d} of {n:4d} = {100 * share:5.2f} % "
                      f"(cap {100 * C.CAPS[entry]:.0f} %)")
            assert share <= C.CAPS[entry], (entry, label, b, n)
        if rows:
            out["screened/" + entry] = np.array([[b, n] for _, b, n in rows], np.int32)
    return out


def main(path=C.FIXTURE):
    if not reflib.available():
        sys.exit("oracle/_ref/libgbp_ref.so is missing: run build() where the reference's sources are")
    arrays = generate()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.0f} kB, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
