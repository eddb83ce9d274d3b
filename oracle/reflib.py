"""ctypes binding of the compiled reference (oracle/_ref/libgbp_ref.so).

TEST INFRASTRUCTURE ONLY.  The library is the reference planner's own seven
ROS-free sources plus oracle/ref/ref_driver.cpp, built by `make -C oracle ref`
where the reference's sources are present; it is never committed.  Only
tools/make_ref_golden.py and the live leg of tests/test_reference_parity.py
load it.  No GPU test, smoke() or bench.py may.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libgbp_ref.so")

_lib = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB_PATH)
        P, I, D, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
        sig = {
            "ref_terrain_new": (P, [I, I, P, P, P, P, P, P]),
            "ref_terrain_free": (None, [P]),
            "ref_lookups": (None, [P, I64, P, P, P, P]),
            "ref_apply": (None, [I64, P, P, P, P]),
            "ref_distances": (None, [I64, P, P, D, D, P, P]),
            "ref_valid_actions": (None, [I64, P, P]),
            "ref_rotate_grf": (None, [I64, P, P, P]),
            "ref_interp": (None, [I64, P, P, P, P]),
            "ref_interp_path": (I, [I, P, P, D, I, P, P, P]),
            "ref_valid_states": (None, [P, I64, P, I, P]),
            "ref_pairs": (None, [P, I64, P, P, P, I, P, P, P]),
            "ref_connects": (None, [P, I64, P, P, P, P, I, P, P, P]),
            "ref_tree_new": (P, [P, I, D, D]),
            "ref_tree_free": (None, [P]),
            "ref_tree_size": (I, [P]),
            "ref_tree_add": (None, [P, I, P, I, P]),
            "ref_tree_update_gy": (None, [P, I, D, D]),
            "ref_tree_dump": (None, [P, I, P, P, P, P, P]),
            "ref_tree_nearest": (None, [P, I64, P, P]),
            "ref_tree_neighborhood_dist": (I, [P, P, D, I, P]),
            "ref_tree_neighborhood_n": (I, [P, P, I, P]),
            "ref_tree_connect": (I, [P, P, P, I, I]),
            "ref_tree_path": (I, [P, I, P, P, P, P]),
            "ref_join": (I, [P, P, I, I, P, P]),
            "ref_post_process": (I, [P, I, P, P, I, I, D, D, P, P, P]),
            "ref_srand": (None, [ctypes.c_uint]),
            "ref_extend": (I, [P, P, P, I, I, I]),
        }
        for name, (res, args) in sig.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype=np.float64):
    return np.ascontiguousarray(a, dtype=dtype)


class RefTerrain:
    """FastTerrainMap loaded through its own loadData (x-major arrays)."""

    def __init__(self, x, y, z, dx=None, dy=None, dz=None):
        x, y, z = _c(x), _c(y), _c(z)
        nx, ny = x.size, y.size
        dx = np.zeros((nx, ny)) if dx is None else _c(dx)
        dy = np.zeros((nx, ny)) if dy is None else _c(dy)
        dz = np.ones((nx, ny)) if dz is None else _c(dz)
        self.h = lib().ref_terrain_new(nx, ny, _p(x), _p(y), _p(z), _p(dx), _p(dy), _p(dz))

    @classmethod
    def from_data(cls, td):
        return cls(td.x, td.y, td.z, td.dx, td.dy, td.dz)

    def __del__(self):
        if self.h and _lib is not None:
            _lib.ref_terrain_free(self.h)
            self.h = None

    def lookups(self, xy):
        xy = _c(xy).reshape(-1, 2)
        n = xy.shape[0]
        h, nan, nrm = np.empty(n), np.empty(n, np.uint8), np.empty((n, 3))
        lib().ref_lookups(self.h, n, _p(xy), _p(h), _p(nan), _p(nrm))
        return h, nan, nrm

    def valid_states(self, s, phase):
        s = _c(s).reshape(-1, 8)
        out = np.empty(s.shape[0], np.uint8)
        lib().ref_valid_states(self.h, s.shape[0], _p(s), int(phase), _p(out))
        return out

    def pairs(self, s, a, direction, adaptive, s_new_init, t_new_init):
        s, a = _c(s).reshape(-1, 8), _c(a).reshape(-1, 10)
        n = s.shape[0]
        d = _c(np.broadcast_to(direction, n), np.uint8)
        valid = np.empty(n, np.uint8)
        s_new = np.broadcast_to(_c(s_new_init), (n, 8)).copy()
        t_new = np.broadcast_to(_c(t_new_init), n).copy()
        lib().ref_pairs(self.h, n, _p(s), _p(a), _p(d), int(bool(adaptive)), _p(valid), _p(s_new),
                        _p(t_new))
        return valid, s_new, t_new

    def connects(self, s_existing, s, direction, adaptive, t_s=None):
        """attemptConnect; t_s None: the two-state overload."""
        e, s = _c(s_existing).reshape(-1, 8), _c(s).reshape(-1, 8)
        n = e.shape[0]
        d = _c(np.broadcast_to(direction, n), np.uint8)
        ts = np.full(n, np.nan) if t_s is None else _c(np.broadcast_to(t_s, n)).copy()
        res = np.empty(n, np.int32)
        s_new, a_new = np.full((n, 8), np.nan), np.full((n, 10), np.nan)
        lib().ref_connects(self.h, n, _p(e), _p(s), _p(ts), _p(d), int(bool(adaptive)), _p(res),
                           _p(s_new), _p(a_new))
        return res, s_new, a_new

    def post_process(self, states, actions, adaptive=False, yaw=None):
        """postProcessPath -> (states, actions, [length, yaw, cost]); yaw: None
        or (length_weight, yaw_weight) for cost_add_yaw."""
        st, ac = _c(states).reshape(-1, 8), _c(actions).reshape(-1, 10)
        n = st.shape[0]
        os_, oa, fig = np.zeros((n, 8)), np.zeros((max(n - 1, 1), 10)), np.zeros(3)
        lw, yw = yaw if yaw is not None else (1.0, 1.0)
        m = lib().ref_post_process(self.h, n, _p(st), _p(ac), int(bool(adaptive)),
                                   int(yaw is not None), float(lw), float(yw), _p(os_), _p(oa),
                                   _p(fig))
        return os_[:m].copy(), oa[:m - 1].copy(), fig


class RefTree:
    """A PlannerClass tree (GraphClass::init / addVertex / addEdge / addAction)."""

    def __init__(self, root, yaw=None):
        lw, yw = yaw if yaw is not None else (1.0, 1.0)
        self.h = lib().ref_tree_new(_p(_c(root)), int(yaw is not None), float(lw), float(yw))

    def __del__(self):
        if self.h and _lib is not None:
            _lib.ref_tree_free(self.h)
            self.h = None

    @property
    def n(self):
        return lib().ref_tree_size(self.h)

    def add(self, idx, s, parent, a):
        lib().ref_tree_add(self.h, int(idx), _p(_c(s)), int(parent), _p(_c(a)))

    def update_gy(self, idx, g, y):
        lib().ref_tree_update_gy(self.h, int(idx), float(g), float(y))

    def dump(self):
        n = self.n
        v, a = np.empty((n, 8)), np.empty((n, 10))
        parent, g, y = np.empty(n, np.int32), np.empty(n), np.empty(n)
        lib().ref_tree_dump(self.h, n, _p(v), _p(a), _p(parent), _p(g), _p(y))
        return dict(v=v, act=a, parent=parent, g=g, y=y)

    def nearest(self, q):
        q = _c(q).reshape(-1, 8)
        out = np.empty(q.shape[0], np.int32)
        lib().ref_tree_nearest(self.h, q.shape[0], _p(q), _p(out))
        return out

    def neighborhood_dist(self, q, dist):
        out = np.empty(self.n, np.int32)
        m = lib().ref_tree_neighborhood_dist(self.h, _p(_c(q)), float(dist), out.size, _p(out))
        return out[:m].copy()

    def neighborhood_n(self, q, k):
        out = np.empty(max(self.n, 1), np.int32)
        m = lib().ref_tree_neighborhood_n(self.h, _p(_c(q)), int(k), _p(out))
        return out[:m].copy()

    def connect(self, terrain, s, direction, adaptive=False):
        return lib().ref_tree_connect(self.h, terrain.h, _p(_c(s)), int(direction),
                                      int(bool(adaptive)))

    def extend(self, terrain, target, direction, adaptive=False, star=True):
        return lib().ref_extend(self.h, terrain.h, _p(_c(target)), int(direction),
                                int(bool(adaptive)), int(bool(star)))

    def path(self, idx):
        n = self.n
        path, st = np.empty(n, np.int32), np.empty((n, 8))
        ac, ar = np.empty((n, 10)), np.empty((n, 10))
        m = lib().ref_tree_path(self.h, int(idx), _p(path), _p(st), _p(ac), _p(ar))
        return path[:m].copy(), st[:m].copy(), ac[:m - 1].copy(), ar[:m - 1].copy()


def join(ta, tb, ia, ib):
    n = ta.n + tb.n
    st, ac = np.empty((n, 8)), np.empty((n, 10))
    m = lib().ref_join(ta.h, tb.h, int(ia), int(ib), _p(st), _p(ac))
    return st[:m].copy(), ac[:m - 1].copy()


def apply(s, a, t):
    s, a, t = _c(s).reshape(-1, 8), _c(a).reshape(-1, 10), _c(t).ravel()
    out = np.empty((s.shape[0], 6, 8))
    lib().ref_apply(s.shape[0], _p(s), _p(a), _p(t), _p(out))
    return out


def distances(q1, q2, lw, yw):
    q1, q2 = _c(q1).reshape(-1, 8), _c(q2).reshape(-1, 8)
    out, within = np.empty((q1.shape[0], 5)), np.empty(q1.shape[0], np.uint8)
    lib().ref_distances(q1.shape[0], _p(q1), _p(q2), float(lw), float(yw), _p(out), _p(within))
    return out, within


def valid_actions(a):
    a = _c(a).reshape(-1, 10)
    out = np.empty(a.shape[0], np.uint8)
    lib().ref_valid_actions(a.shape[0], _p(a), _p(out))
    return out


def rotate_grf(nrm, f):
    nrm, f = _c(nrm).reshape(-1, 3), _c(f).reshape(-1, 3)
    out = np.empty_like(f)
    lib().ref_rotate_grf(f.shape[0], _p(nrm), _p(f), _p(out))
    return out


def interp(q1, q2, x):
    q1, q2, x = _c(q1).reshape(-1, 8), _c(q2).reshape(-1, 8), _c(x).ravel()
    out = np.empty_like(q1)
    lib().ref_interp(q1.shape[0], _p(q1), _p(q2), _p(x), _p(out))
    return out


def interp_path(states, actions, dt, cap=20000):
    st, ac = _c(states).reshape(-1, 8), _c(actions).reshape(-1, 10)
    path, t, ph = np.empty((cap, 8)), np.empty(cap), np.empty(cap, np.int32)
    m = lib().ref_interp_path(st.shape[0], _p(st), _p(ac), float(dt), cap, _p(path), _p(t), _p(ph))
    assert m > 0, m
    return path[:m].copy(), t[:m].copy(), ph[:m - 1].copy()


def srand(seed):
    lib().ref_srand(int(seed))
