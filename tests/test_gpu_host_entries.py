"""The host-pointer entry points (`gbp_*_host`) against their `_dev` entries.

A `_host` entry states its device arrays once, as a list the staging helper
runs twice (sizing, then carving): the workspace is sized by the same list
that hands out the pointers.  Bar: every output of a `_host` entry equals the
matching `_dev` entry's bit for bit on the same inputs.

Terrain-handle entries: on one fresh handle (synth-rough-256) each entry runs
with n = 1, 300, 70,000, 1.  At 1 and 300 the workspace sits at its 1 MiB
floor; 70,000 is past the floor for every entry (the smallest footprint is
height's 26 B per item, 1.8 MB), and the entries are listed by ascending
footprint, so each one's 70,000 regrows the workspace and its final 1 reuses
the grown buffer.  The `_dev` references run on a second handle of the same
terrain, so the fresh handle's workspace sees the host entries only.  The
three entries that re-decide FRAGILE results on the host (valid_states,
validate_pairs, extend_batch) are compared after the matching
gbp_*resolve*_host call on the device results; for validate_pairs the FRAGILE
attempts' s_new / t_new are first put back to the caller's contents, as
gbp_validate_pairs_host documents.

Terrain-less entries (a scoped device buffer of their own): n_query in
{1, 300} x n_vert in {0, 1, 1000}, n_nearest in {1, GBP_KNN_MAX}, max_out in
{0, 8}.  gbp_neighbors_batch_dev assigns out[i] only up to count[i], so that
is what is compared there.

Outputs are pre-filled with NaN / 7, and every host output array has four
spare rows behind it that must keep the fill.
"""
import ctypes

import numpy as np
import pytest

from global_body_planner_amd import _lib as L
from global_body_planner_amd import terrain_data as td
from global_body_planner_amd import workload as W

torch = pytest.importorskip("torch")

VP = ctypes.c_void_p
N_MAX = 70000
SIZES = (1, 300, N_MAX, 1)
SEED, STREAM, BASE = 97, 11, 5
GUARD = 4
KNN_MAX = 64
_cache = {}


def hp(a):
    return None if a is None else a.ctypes.data_as(VP)


def dp(t):
    return None if t is None else VP(t.data_ptr())


def filled(rows, tail, dtype):
    """rows x tail of NaN (floating) or 7."""
    return np.full((rows,) + tail, np.nan if np.dtype(dtype).kind == "f" else 7, dtype)


def to_dev(a):
    """A device copy of a numpy array (uint32 travels as int32: same bits)."""
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def setup():
    """Made once: the fresh handle, the reference handle, N_MAX rows of every input on both sides."""
    if not _cache:
        import global_body_planner_amd as gbp
        data = td.by_name("synth-rough-256")
        ref = gbp.Terrain.from_data(data, device=0)
        s, a, d, target, _ = W.make_attempts(ref, N_MAX, 4242)
        nrm, _ = ref.normal(target[:, :2])
        dev = dict(s=s.contiguous(), a=a.contiguous(), d=d.contiguous(), target=target.contiguous(),
                   xy=target[:, :2].contiguous(), nrm=nrm.contiguous())
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in dev.items()}
        lib = L.load()
        q, v = host["s"][:300], host["target"][:1000]
        host["qy"] = np.array([lib.gbp_host_yaw(hp(q[i:i + 1])) for i in range(len(q))])
        host["vy"] = np.array([lib.gbp_host_yaw(hp(v[i:i + 1])) for i in range(len(v))])
        dev["qy"], dev["vy"] = to_dev(host["qy"]), to_dev(host["vy"])
        # a radius that gives query 0 about twenty neighbours among the 1000 vertices
        radius = float(np.sort(np.sqrt(((v - q[0]) ** 2).sum(1)))[20])
        _cache.update(lib=lib, ref=ref, fresh=gbp.Terrain.from_data(data, device=0), dev=dev,
                      host=host, radius=radius)
    return _cache


# ---- terrain-handle entries -------------------------------------------------------
U1, I4, U4, F8 = np.uint8, np.int32, np.uint32, np.float64
CFG = L.sampling(state_flag=True, state_p=0.5, action_flag=True, action_p=0.5)
S_FROM = np.array([1.0, 2.5, 0.3, 0.5, 0.1, 0.0, 0.0, 0.0])
S_TO = np.array([4.0, 2.6, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0])

# name -> (outputs [(name, row tail, dtype)], arguments behind (t, n) from inputs i and outputs o,
#          the host re-decision of the device results or None); by ascending bytes per item
ENTRIES = {
    "height_batch": (
        [("h", (), F8), ("nan", (), U1), ("ood", (), U1)],
        lambda i, o: (i["xy"], o["h"], o["nan"], o["ood"]), None),
    "normal_batch": (
        [("nrm", (3,), F8), ("ood", (), U1)],
        lambda i, o: (i["xy"], o["nrm"], o["ood"]), None),
    "sample_states_dir": (
        [("states", (8,), F8)],
        lambda i, o: (SEED, STREAM, BASE, ctypes.byref(CFG), hp(S_FROM), hp(S_TO), o["states"]), None),
    "sample_states": (
        [("states", (8,), F8), ("tries", (), I4)],
        lambda i, o: (SEED, STREAM, BASE, L.STANCE, 8, o["states"], o["tries"]), None),
    "valid_states": (
        [("valid", (), U1), ("flags", (), U4), ("counts", (), U4)],
        lambda i, o: (i["s"], i["d"], 0, o["valid"], o["flags"], o["counts"]),
        "gbp_resolve_fragile_states_host"),
    "sample_actions": (
        [("actions", (10,), F8)],
        lambda i, o: (i["nrm"], SEED, STREAM, BASE, o["actions"]), None),
    "validate_pairs": (
        [("valid", (), U1), ("s_new", (8,), F8), ("t_new", (), F8), ("flags", (), U4), ("counts", (), U4)],
        lambda i, o: (i["s"], i["a"], i["d"], 0, 0, o["valid"], o["s_new"], o["t_new"], o["flags"],
                      o["counts"]),
        "gbp_resolve_fragile_host"),
    "sample_actions_dir": (
        [("actions", (10,), F8)],
        lambda i, o: (i["nrm"], i["target"], i["s"], i["d"], 0, ctypes.byref(CFG), SEED, STREAM, BASE,
                      o["actions"]), None),
    "extend_batch": (
        [("result", (), I4), ("chosen", (), I4), ("s_new", (8,), F8), ("a_new", (10,), F8),
         ("counts", (), U4), ("flags", (), U4)],
        lambda i, o: (i["s"], i["target"], i["d"], 0, 0, SEED, BASE, o["result"], o["chosen"],
                      o["s_new"], o["a_new"], o["counts"], o["flags"]),
        "gbp_extend_resolve_host"),
}


def run_entry(name, n):
    """(host results, device results re-decided as the host entry does), each {output: numpy [n, ...]}."""
    c = setup()
    lib, outs, args, resolve = c["lib"], *ENTRIES[name]
    stream = VP(torch.cuda.current_stream(0).cuda_stream)
    with_t = name != "sample_actions"   # gbp_sample_actions_dev takes no handle

    # the device entry on the reference handle
    dout = {k: to_dev(filled(n, tail, dt)) for k, tail, dt in outs}
    dargs = args({k: dp(v) for k, v in c["dev"].items()}, {k: dp(v) for k, v in dout.items()})
    rc = getattr(lib, f"gbp_{name}_dev")(*((c["ref"]._h,) if with_t else ()), n, *dargs, stream)
    assert rc == 0, (name, n, rc)
    torch.cuda.synchronize()
    want = {k: to_host(dout[k], dt) for k, _, dt in outs}
    hin = {k: hp(v) for k, v in c["host"].items()}
    if resolve:
        if name == "validate_pairs":   # the caller's contents back for the attempts re-decided
            frag = (want["flags"] & L.F_FRAGILE) != 0
            want["s_new"][frag] = np.nan
            want["t_new"][frag] = np.nan
        rc = getattr(lib, resolve)(c["ref"]._h, n, *args(hin, {k: hp(v) for k, v in want.items()}), None)
        assert rc == 0, (name, n, resolve, rc)

    # the host entry on the fresh handle, four guard rows behind every output
    hout = {k: filled(n + GUARD, tail, dt) for k, tail, dt in outs}
    rc = getattr(lib, f"gbp_{name}_host")(c["fresh"]._h, n, *args(hin, {k: hp(v) for k, v in hout.items()}))
    assert rc == 0, (name, n, rc)
    for k, tail, dt in outs:
        assert np.array_equal(raw(hout[k][n:]), raw(filled(GUARD, tail, dt))), \
            f"{name} n={n}: {k} written past its {n} rows"
    return {k: v[:n] for k, v in hout.items()}, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENTRIES))
def test_terrain_entry(gpu, name):
    for n in SIZES:
        got, want = run_entry(name, n)
        for k in want:
            bad = np.flatnonzero((raw(got[k]).reshape(n, -1) != raw(want[k]).reshape(n, -1)).any(1))
            assert bad.size == 0, f"{name} n={n}: {k} differs from the device entry at rows {bad[:10]}"


# ---- terrain-less entries ---------------------------------------------------------
SHAPES = [(nq, nv) for nq in (1, 300) for nv in (0, 1, 1000)]


def tree_inputs(nq, nv):
    """Host and device pointers of nq queries and nv vertices (null for an empty tree), with their yaws."""
    c = setup()
    h, d = c["host"], c["dev"]
    return (dict(q=hp(h["s"]), v=hp(h["target"]) if nv else None),
            dict(q=dp(d["s"]), v=dp(d["target"]) if nv else None, qy=dp(d["qy"]),
                 vy=dp(d["vy"]) if nv else None))


def both(name, nq, outs, hargs, dargs):
    """The host and the device entry on sentinel-filled outputs: ({output: host rows}, {output: device rows})."""
    lib = setup()["lib"]
    hout = {k: filled(nq + GUARD, tail, dt) for k, tail, dt in outs}
    dout = {k: to_dev(filled(nq, tail, dt)) for k, tail, dt in outs}
    rc = getattr(lib, f"gbp_{name}_host")(*hargs({k: hp(v) for k, v in hout.items()}))
    assert rc == 0, (name, rc)
    rc = getattr(lib, f"gbp_{name}_dev")(*dargs({k: dp(v) for k, v in dout.items()}),
                                         VP(torch.cuda.current_stream(0).cuda_stream))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    for k, tail, dt in outs:
        assert np.array_equal(raw(hout[k][nq:]), raw(filled(GUARD, tail, dt))), \
            f"{name}: {k} written past its {nq} rows"
    return {k: v[:nq] for k, v in hout.items()}, {k: to_host(dout[k], dt) for k, _, dt in outs}


def assert_rows_equal(got, want, label):
    for k in want:
        assert np.array_equal(raw(got[k]), raw(want[k])), f"{label}: {k} differs from the device entry"


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nv", SHAPES)
def test_nearest(gpu, nq, nv):
    h, d = tree_inputs(nq, nv)
    got, want = both("nearest_batch", nq, [("index", (), I4), ("dist", (), F8)],
                     lambda o: (nq, h["q"], nv, h["v"], o["index"], o["dist"]),
                     lambda o: (nq, d["q"], nv, d["v"], o["index"], o["dist"]))
    assert_rows_equal(got, want, f"nearest {nq}x{nv}")


@pytest.mark.gpu
@pytest.mark.parametrize("nq,nv", SHAPES)
def test_neighbors(gpu, nq, nv):
    h, d = tree_inputs(nq, nv)
    radius = setup()["radius"]
    for max_out in (0, 8):
        outs = [("out", (max_out,), I4), ("count", (), I4)]
        got, want = both("neighbors_batch", nq, outs,
                         lambda o: (nq, h["q"], nv, h["v"], radius, max_out, o["out"] if max_out else None,
                                    o["count"]),
                         lambda o: (nq, d["q"], nv, d["v"], radius, max_out, o["out"] if max_out else None,
                                    o["count"]))
        label = f"neighbors {nq}x{nv} max_out={max_out}"
        assert np.array_equal(got["count"], want["count"]), f"{label}: count differs"
        assert (got["count"] >= 0).all() and (got["count"] <= nv).all(), label
        if nv == 1000:
            assert got["count"][0] > 8, f"{label}: the radius should overflow max_out for query 0"
        assigned = np.arange(max_out)[None, :] < got["count"][:, None]
        assert np.array_equal(got["out"][assigned], want["out"][assigned]), f"{label}: out differs"
        assert (want["out"][~assigned] == 7).all(), label


@pytest.mark.gpu
@pytest.mark.parametrize("yaw", [False, True])
@pytest.mark.parametrize("nq,nv", SHAPES)
def test_knn(gpu, nq, nv, yaw):
    h, d = tree_inputs(nq, nv)
    lw, yw = 1.25, 0.5
    for k in (1, KNN_MAX):
        outs = [("out", (k,), I4), ("dist", (k,), F8)]
        if yaw:   # the yaws the host entry forms with gbp_host_yaw, handed to the device entry
            got, want = both("knn_yaw_batch", nq, outs,
                             lambda o: (nq, h["q"], nv, h["v"], lw, yw, k, o["out"], o["dist"]),
                             lambda o: (nq, d["q"], d["qy"], nv, d["v"], d["vy"], lw, yw, k, o["out"],
                                        o["dist"]))
        else:
            got, want = both("knn_batch", nq, outs,
                             lambda o: (nq, h["q"], nv, h["v"], k, o["out"], o["dist"]),
                             lambda o: (nq, d["q"], nv, d["v"], k, o["out"], o["dist"]))
        assert_rows_equal(got, want, f"knn yaw={yaw} {nq}x{nv} k={k}")
        assert ((got["out"] >= 0).sum(1) == min(k, nv)).all()
