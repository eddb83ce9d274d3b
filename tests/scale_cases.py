"""Inputs shared by the tests that run the engine past one grid pass
(test_scale_cases.py on the CPU, test_gpu_tree_scale.py, test_gpu_batch_scale.py
and the many-window cases of test_gpu_shortcut.py on the GPU), each computed
once per process:

  * the big tree: 745 copies of set S's tree a under its root, 70,031 vertices
    with real edges and 745-way ties in f, plain and renumbered, and its edge
    decisions on box 1 (the 95-vertex tree's, tiled as the vertices are);
  * a random recursive tree of the same size, renumbered, with seeded edge
    decisions and attach flags: the input of re-root and graft;
  * the key-range tree: a star whose f values are +0, 2e-150 .. 2e150, values
    that differ in their low bytes alone, +inf and NaN, with the budgets that
    make every round of the trim's radix select choose among several bytes;
  * windows of the densified paths of tests/shortcut_cases.py: more paths in
    one shortcut call than a launch takes.

The grid caps restated here are the launch code's (csrc/gbp_tree_maint.hip,
gbp_tree_trim.hip, gbp_engine.hip) at 256 CUs; with fewer CUs they are lower.
"""
import functools

import numpy as np

from tests import prune_ref as R
from tests import reroot_ref as RR
from tests import shared_ref as SR
from tests import shortcut_cases as C
from tests import trim_ref as TR

CUS = 256
TB = 256                       # threads of a workgroup in every kernel named below
PRUNE_PIECES = 9               # pieces of a vertex k_prune_gather / k_prune_move_rows move
CAP_GATHER = 8 * CUS           # k_prune_gather's workgroups at most
CAP_MOVE_ROWS = 2048           # k_prune_move_rows'
TRIM_HIST_GRID = 128           # k_trim_hist's
COPIES = 745
N_BIG = 94 * COPIES + 1        # 70,031
PERMUTE_SEED = 20251020
CHUNK = 262144                 # the batch test_gpu_parity.py pins to the oracle
N_EXTEND_PREP = 175003         # 6 n candidates: past k_extend_prep's 16 x CUs x 256


def batch_n(cus):
    """One element past two turns' boundary of a 16 x CUs grid of 256, and a
    last workgroup that is not full."""
    return 16 * cus * 256 + 256 + 37


# ---- the big tree -------------------------------------------------------------------------
def renumbering(n, seed):
    """old index -> new index of test_gpu_tree_prune._permuted / reroot_ref.permuted."""
    return np.r_[0, 1 + np.random.default_rng(seed).permutation(n - 1)]


def tiled(x, copies=COPIES):
    """A per-vertex array of the 95-vertex tree, laid out as _copies lays out the vertices."""
    return np.concatenate([x[:1]] + [x[1:]] * copies)


@functools.lru_cache(maxsize=None)
def big_tree(permute=False):
    """(tree of 70,031 vertices, the goal root its f is taken toward, set S's best cost)."""
    from tests.test_gpu_tree_prune import _copies, _permuted
    r = R.search("S")
    t = _copies(r["a"], COPIES)
    if permute:
        t = _permuted(t, PERMUTE_SEED)
    for a in t.values():
        a.setflags(write=False)
    return t, r["b"]["v"][0], r["best_cost"]


@functools.lru_cache(maxsize=None)
def big_edge_valid(permute=False):
    """The big tree's edge decisions on box 1: a copy's edge has the states and
    the action of the edge it copies, so the 95 decisions are tiled."""
    _, O = R.terrain("box1")
    ok = tiled(R.edge_valid(O, R.search("S")["a"], R.FORWARD))
    if permute:
        out = np.empty_like(ok)
        out[renumbering(N_BIG, PERMUTE_SEED)] = ok
        ok = out
    ok.setflags(write=False)
    return ok


def depths(parent):
    """Edges between each vertex and the root: a fixed point, no walk per vertex."""
    parent = np.asarray(parent)
    d = np.zeros(len(parent), np.int64)
    while True:
        nxt = d.copy()
        nxt[1:] = d[parent[1:]] + 1
        if np.array_equal(nxt, d):
            return d
        d = nxt


def deepest(tree, f):
    """Of the vertices the most edges from the root, the first of the largest f."""
    d = depths(tree["parent"])
    far = np.flatnonzero(d == d.max())
    return int(far[np.argmax(np.asarray(f)[far])])


def sample_of(n, seed, count=2000, ends=300):
    """The first and last `ends` indices and `count` random ones: where the
    tiled edge decisions are compared with the oracle's own."""
    if n <= count + 2 * ends:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    return np.unique(np.r_[np.arange(ends), np.arange(n - ends, n), rng.integers(0, n, count)])


BIG_BUDGETS = (1, 32769, 40000, N_BIG - 1)


@functools.lru_cache(maxsize=None)
def big_bound():
    """A bound half way between the cuts of the budgets 32,769 and 40,000:
    with the smaller budget both tests drop vertices."""
    tree, rb, _ = big_tree()
    f = np.sort(TR.f_values(tree, rb)[1:])
    return float((f[32768] + f[39999]) / 2)


# ---- the random recursive tree ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_tree():
    """(tree, k, edge decisions, attach flags, connect actions): 70,031 vertices
    with parent[i] drawn below i, renumbered so that parents follow children; k
    the non-root vertex that heads the most vertices; about 2 % of the edges
    fail and 1 % of the vertices are attached, by seeded draws."""
    plain = RR.random_recursive_tree(N_BIG, seed=20261120)
    size = np.ones(N_BIG, np.int64)
    p = plain["parent"]
    for i in range(N_BIG - 1, 0, -1):      # parents precede children here
        size[p[i]] += size[i]
    k0 = 1 + int(np.argmax(size[1:]))
    tree, k = RR.permuted(plain, k0, 20261121)
    ok = (np.random.default_rng(20261122).random(N_BIG) >= 0.02).astype(np.uint8)
    attach = (np.random.default_rng(20261123).random(N_BIG) < 0.01).astype(np.uint8)
    actions = np.random.default_rng(20261124).uniform(-1.0, 1.0, (N_BIG, 10))
    return tree, k, ok, attach, actions, int(size[k0])


NEW_ROOT = np.array([0.25, -0.5, 0.75, 0.1, -0.2, 0.3, 0.05, -0.05])


# ---- the key-range tree ------------------------------------------------------------------
def trim_keys(f):
    """The order-preserving 64-bit image of f the select sorts by, restated:
    -0 taken as +0, the sign bit set on a positive value, a negative one
    inverted, every NaN the largest key."""
    f = np.array(f, np.float64)
    f[f == 0.0] = 0.0
    b = f.view(np.uint64)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    k[np.isnan(f)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def select_rounds(keys, max_keep):
    """The eight rounds of the select for the budget max_keep over keys (the
    non-root vertices'): per round the number of byte values that occur among
    the keys sharing the bytes fixed so far.  -> (occupied [8], the cut's key)"""
    keys = np.asarray(keys, np.uint64)
    rank = max_keep - 1
    live = np.ones(len(keys), bool)
    occupied = []
    prefix = np.uint64(0)
    for shift in range(56, -8, -8):
        digit = ((keys >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        cnt = np.bincount(digit[live], minlength=256)
        occupied.append(int((cnt > 0).sum()))
        before = np.cumsum(cnt) - cnt
        d = int(np.flatnonzero((before <= rank) & (rank < before + cnt))[0])
        rank -= int(before[d])
        live &= digit == d
        prefix |= np.uint64(d) << np.uint64(shift)
    return occupied, prefix


def _low_byte_run(rng, count, nbytes, top_bits):
    """count values 1 + k 2^-52, k < 2^(8 nbytes + top_bits): every byte of k
    is one of four values fixed per position, so that many k share a prefix
    and part at every byte below it."""
    k = np.zeros(count, np.uint64)
    k |= rng.choice(rng.permutation(1 << top_bits)[:4], count).astype(np.uint64) << np.uint64(8 * nbytes)
    for b in range(nbytes):
        k |= rng.choice(rng.permutation(256)[:4], count).astype(np.uint64) << np.uint64(8 * b)
    return 1.0 + k.astype(np.float64) * 2.0 ** -52, k


@functools.lru_cache(maxsize=None)
def key_tree():
    """(tree, the other tree's root, x): a star under a root at the origin,
    v[i] = (x_i, 0, ...), toward a root at the origin: g_i = |x_i| and
    f_i = 2 |x_i| exactly wherever x_i^2 neither overflows nor underflows.  x
    holds exact zeros, +-10^e with e uniform in [-150, 150], a run at 1e200
    (the square overflows: f = +inf), a run of +-inf, a run of NaN, and two
    runs 1 + k 2^-52 with k < 2^20 and k < 2^44; every run holds exact
    duplicates.  The order is shuffled."""
    rng = np.random.default_rng(20261130)
    mags = 10.0 ** rng.uniform(-150.0, 150.0, 560) * rng.choice([-1.0, 1.0], 560)
    run20, k20 = _low_byte_run(rng, 330, 2, 4)
    run44, k44 = _low_byte_run(rng, 400, 5, 4)
    assert k20.max() < 1 << 20 and k44.max() < 1 << 44
    parts = [np.zeros(6), -np.zeros(2), mags, mags[:20],
             np.full(36, 1e200) * rng.choice([-1.0, 1.0], 36),
             np.full(36, np.inf) * rng.choice([-1.0, 1.0], 36),
             np.full(40, np.nan), run20, run20[:15], run44, run44[:15]]
    x = rng.permutation(np.concatenate(parts))
    n = 1 + len(x)
    v = np.zeros((n, 8))
    v[1:, 0] = x
    act = rng.uniform(-1.0, 1.0, (n, 10))
    act[0] = 0.0
    parent = np.r_[-1, np.zeros(n - 1)].astype(np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        g = SR.pose_g(v, parent)
    return dict(v=v, act=act, parent=parent, g=g), np.zeros(8), x


def quiet(fn, *args):
    """fn(*args) with numpy's overflow and invalid-value warnings off: the
    key-range tree's squares overflow and its NaN compare on purpose."""
    with np.errstate(over="ignore", invalid="ignore"):
        return fn(*args)


def key_f():
    tree, root, _ = key_tree()
    return quiet(TR.f_values, tree, root)


@functools.lru_cache(maxsize=None)
def key_budgets():
    """name -> max_keep.  The cut of a budget is the (max_keep - 1)-th of the
    sorted non-root f: the named budgets put it on +0, inside a run of equal
    values, on +inf and on NaN; the others inside the two low-byte runs and
    among the magnitudes, where the select's rounds part."""
    f = np.sort(key_f()[1:])           # NaN last, above +inf
    n = len(f) + 1
    zero = int((f == 0).sum())
    fin = int(np.isfinite(f).sum())
    inf = int(np.isinf(f).sum())
    lo, hi = (int(np.searchsorted(f, 2.0, side=s)) for s in ("left", "right"))
    end = int(np.searchsorted(f, 2.0 + 2.0 ** -7))          # past both runs (k < 2^44)
    end20 = int(np.searchsorted(f, 2.0 + 2.0 ** -31))       # past the run k < 2^20
    assert zero >= 8 and lo <= hi < end20 < end
    tie = next(i for i in range((hi + end20) // 2, end20) if f[i] == f[i + 1])
    out = {"zero": 1, "zero-tie": zero - 2, "low": zero + (lo - zero) // 3, "n-1": n - 1,
           "tie": tie + 1, "inf": fin + inf // 2 + 1, "nan": fin + inf + 20 + 1,
           "high": end + (fin - end) // 2}
    for j in range(1, 5):
        out[f"run20-{j}"] = hi + (end20 - hi) * j // 5 + 1
        out[f"run44-{j}"] = end20 + (end - end20) * j // 5 + 1
    return out


def key_cut(max_keep):
    return float(np.sort(key_f()[1:])[max_keep - 1])


# ---- path windows ---------------------------------------------------------------------------
N_WINDOWS = 150
WINDOW_CALLS = (65, 128, 150)


@functools.lru_cache(maxsize=None)
def windows(dense):
    """[(offset, length)] x 150 of the densified path C.DENSE[dense]: 2 to 12
    consecutive states; the first four are the shortest and the longest at
    both ends of the path."""
    n = len(C.dense_path(*C.DENSE[dense])[0])
    rng = np.random.default_rng(20261140 + dense)
    out = [(0, 2), (n - 2, 2), (0, 12), (n - 12, 12)]
    while len(out) < N_WINDOWS:
        length = int(rng.integers(2, 13))
        out.append((int(rng.integers(0, n - length + 1)), length))
    return tuple(out)


def window_paths(dense):
    """([states], [actions]) of the windows: the dense path's rows and its marker actions."""
    S, A = C.dense_path(*C.DENSE[dense])
    w = windows(dense)
    return [S[o:o + m] for o, m in w], [A[o:o + m - 1] for o, m in w]


def window_block(table, n, offset, length):
    """The window's connect table out of the dense path's packed table of n
    states: a pair's decision depends on its two states and the terrain alone."""
    idx = [i * (2 * n - i - 1) // 2 + (j - i - 1)
           for i in range(offset, offset + length) for j in range(i + 1, offset + length)]
    return np.asarray(table)[idx]
