"""Device-side engine API over the C ABI (torch tensors for HBM residency/streams).

`Terrain` owns one gbp_terrain handle (one GPU).  Every batched call takes
device tensors (float64 AoS states [n, 8] / actions [n, 10]) and enqueues the
HIP kernels on torch's current stream for that device; results are device
tensors.  Host (numpy) variants mirror the `_host` C entry points.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as L
from ._lib import check

_VP = ctypes.c_void_p


def _ptr(t):
    return None if t is None else _VP(t.data_ptr())


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(_VP)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _stream(device):
    return _VP(torch.cuda.current_stream(device).cuda_stream)


@dataclass
class PairResult:
    valid: torch.Tensor     # uint8 [n]
    s_new: torch.Tensor     # float64 [n, 8] (rows untouched where flags lack SNEW_SET)
    t_new: torch.Tensor     # float64 [n]
    flags: torch.Tensor     # int32 view of the uint32 flag word [n]
    counts: torch.Tensor    # int32 view of G | V << 16 [n]


@dataclass
class ExtendResult:
    result: torch.Tensor    # int32 TRAPPED / ADVANCED / REACHED
    chosen: torch.Tensor    # int32 candidate index or -1
    s_new: torch.Tensor
    a_new: torch.Tensor
    counts: torch.Tensor
    flags: torch.Tensor     # int32 view: OR of the executed candidates' flags


class Terrain:
    """A FastTerrainMap resident in HBM (x-major heights, fp32 when lossless)."""

    def __init__(self, x, y, z, dx=None, dy=None, dz=None, device=0,
                 storage=L.STORAGE_AUTO, kernel=None, lib=None):
        self._lib = lib if lib is not None else L.load()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        z = np.ascontiguousarray(z, np.float64)
        if z.shape != (x.size, y.size):
            raise ValueError(f"z must be x-major [{x.size}][{y.size}], got {z.shape}")
        nl = [None if v is None else np.ascontiguousarray(v, np.float64) for v in (dx, dy, dz)]
        h = _VP()
        check(self._lib.gbp_terrain_create(self.device, x.size, y.size, _np_ptr(x), _np_ptr(y),
                                           _np_ptr(z), *[_np_ptr(v) for v in nl], int(storage),
                                           ctypes.byref(h)), "gbp_terrain_create")
        self._h = h
        self.nx, self.ny = x.size, y.size
        if kernel is not None:
            self.set_option(L.OPT_KERNEL, kernel)

    @classmethod
    def from_data(cls, td, **kw):
        return cls(td.x, td.y, td.z, td.dx, td.dy, td.dz, **kw)

    # ---- handle ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.gbp_terrain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        nx, ny, st, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        b = (ctypes.c_double * 4)()
        check(self._lib.gbp_terrain_info(self._h, ctypes.byref(nx), ctypes.byref(ny),
                                         ctypes.byref(st), b, ctypes.byref(dev)), "info")
        return {"nx": nx.value, "ny": ny.value, "storage": st.value, "bounds": tuple(b),
                "device": dev.value}

    def set_option(self, key, value):
        check(self._lib.gbp_terrain_set_option(self._h, int(key), int(value)), "set_option")

    def get_option(self, key):
        v = ctypes.c_int64()
        check(self._lib.gbp_terrain_get_option(self._h, int(key), ctypes.byref(v)), "get_option")
        return v.value

    # ---- heights updated in place ----------------------------------------------
    def update(self, z, ix0=0, iy0=0, dx=None, dy=None, dz=None, layout=L.SRC_F64_XMAJOR,
               shape=None):
        """Replace the heights (and, given all three, the slope layers) of a
        rectangle of cells in place (gbp_terrain_update_*): options, sampling,
        workspaces and PlanWorkspace objects of the handle stay.

        layout SRC_F64_XMAJOR: z (and dx / dy / dz) are float64 [pnx][pny], the
        rectangle's cells from (ix0, iy0).  layout SRC_F32_GRIDMAP: float32
        [NY][ld], ld >= NX, a whole grid_map layer as it lies in memory
        (z[c][r] = layer(r, c), cell (ix, iy) at [NY-1-iy][NX-1-ix]); the
        rectangle is `shape` = (pnx, pny) cells from (ix0, iy0), to the map's
        far corner when None.

        numpy input takes the synchronous host entry (a patch an fp32 handle
        cannot hold raises GbpError with status E_UNSUPPORTED and changes
        nothing).  Device tensors take the device entry on the current torch
        stream and return the int32 status tensor ([0] = 0 applied, 1
        rejected), which is read only after that stream is synchronised."""
        on_dev = isinstance(z, torch.Tensor) and z.is_cuda
        dt_np, dt_t = (np.float32, torch.float32) if layout == L.SRC_F32_GRIDMAP \
            else (np.float64, torch.float64)
        arrs = []
        for v in (z, dx, dy, dz):
            if v is None:
                arrs.append(None)
            elif on_dev:
                arrs.append(v.to(device=self.torch_device, dtype=dt_t).contiguous())
            else:
                arrs.append(np.ascontiguousarray(_np(v), dt_np))
        if arrs[0].ndim != 2 or any(v is not None and v.shape != arrs[0].shape for v in arrs[1:]):
            raise ValueError("z, dx, dy, dz must be 2-D arrays of one shape")
        if layout == L.SRC_F32_GRIDMAP:
            if arrs[0].shape[0] != self.ny:
                raise ValueError(f"a grid_map layer is [{self.ny}][ld], got {tuple(arrs[0].shape)}")
            pnx, pny = shape if shape is not None else (self.nx - ix0, self.ny - iy0)
        else:
            pnx, pny = arrs[0].shape
        rect = L.Rect(int(ix0), int(iy0), int(pnx), int(pny))
        ld = int(arrs[0].shape[1])
        if on_dev:
            status = self._empty(1, torch.int32)
            check(self._lib.gbp_terrain_update_dev(self._h, ctypes.byref(rect), int(layout), ld,
                                                   *[_ptr(v) for v in arrs], _ptr(status),
                                                   _stream(self.device)), "update")
            return status
        check(self._lib.gbp_terrain_update_host(self._h, ctypes.byref(rect), int(layout), ld,
                                                *[_np_ptr(v) for v in arrs]), "update")
        return None

    def move(self, sx, sy, x, y, z, dx=None, dy=None, dz=None, layout=L.SRC_F64_XMAJOR):
        """Move the window by (sx, sy) whole cells in place
        (gbp_terrain_move_host): x, y are the new coordinate vectors (the
        handle's sizes), new cell (ix, iy) keeps what old cell (ix + sx, iy +
        sy) held where the old map has it, and every other cell is read from
        z (and dx / dy / dz, all three or none), the WHOLE new map: float64
        [NX][ld >= NY] for SRC_F64_XMAJOR, a float32 grid_map layer [NY][ld >=
        NX] for SRC_F32_GRIDMAP (as `update`).  Only those cells are read.
        Options, sampling, workspaces and PlanWorkspace objects of the handle
        stay; afterwards it equals a fresh Terrain of the moved arrays.  numpy
        input, synchronous; a refused move (GbpError: E_UNSUPPORTED for a new
        height an fp32 handle cannot hold, E_INVALID_ARG for descending
        coordinates) changes nothing.

        A planner.ReplanSession on this terrain goes on across a move:
        T.move(...) and then session.map_changed(), which prunes what the new
        window no longer holds (see planner.ReplanSession.map_changed)."""
        x = np.ascontiguousarray(_np(x), np.float64)
        y = np.ascontiguousarray(_np(y), np.float64)
        if x.shape != (self.nx,) or y.shape != (self.ny,):
            raise ValueError(f"x, y must have the handle's sizes ({self.nx}, {self.ny})")
        dt = np.float32 if layout == L.SRC_F32_GRIDMAP else np.float64
        arrs = [None if v is None else np.ascontiguousarray(_np(v), dt) for v in (z, dx, dy, dz)]
        ld = 0
        if arrs[0] is not None:
            rows = self.ny if layout == L.SRC_F32_GRIDMAP else self.nx
            if arrs[0].ndim != 2 or arrs[0].shape[0] != rows or \
                    any(v is not None and v.shape != arrs[0].shape for v in arrs[1:]):
                raise ValueError(f"z, dx, dy, dz must be whole maps of one shape [{rows}][ld]")
            ld = int(arrs[0].shape[1])
        check(self._lib.gbp_terrain_move_host(self._h, int(sx), int(sy), _np_ptr(x), _np_ptr(y),
                                              int(layout), ld, *[_np_ptr(v) for v in arrs]),
              "move")

    def read(self, rect=None, copy=0):
        """The heights the device holds (gbp_terrain_read_host), float64
        [nx][ny] of rect = (ix0, iy0, nx, ny), the whole map when None.  A
        height lies in up to two x-pairs: copy 0 / 1 choose which is read."""
        r = L.Rect(0, 0, self.nx, self.ny) if rect is None else L.Rect(*[int(v) for v in rect])
        out = np.empty((max(r.nx, 0), max(r.ny, 0)), np.float64)
        check(self._lib.gbp_terrain_read_host(self._h, ctypes.byref(r), int(copy), _np_ptr(out)),
              "read")
        return out

    # ---- slope layers derived from the heights ------------------------------------
    def derive_slopes(self, rect=None, round_f32=False, stream=None):
        """Recompute the slope layers of rect = (ix0, iy0, nx, ny), the whole
        map when None, from the heights the handle holds
        (gbp_terrain_derive_slopes_*, the rule of csrc/gbp_slopes.h).
        round_f32 rounds each component through float last (SLOPES_F32).

        stream None: the synchronous host entry; a handle created without
        layers gets them, (0, 0, 1) outside rect.  A torch stream (or a raw
        stream pointer) selects the device entry, which only enqueues there
        and needs a handle that has layers.

        To keep the layers derived across update / move calls that bring no
        layers: set_option(OPT_DERIVE_SLOPES, 1 | flags)."""
        r = None if rect is None else L.Rect(*[int(v) for v in rect])
        rp = None if r is None else ctypes.byref(r)
        flags = L.SLOPES_F32 if round_f32 else 0
        if stream is None:
            check(self._lib.gbp_terrain_derive_slopes_host(self._h, rp, flags), "derive_slopes")
        else:
            sp = _VP(stream.cuda_stream) if hasattr(stream, "cuda_stream") else _VP(int(stream))
            check(self._lib.gbp_terrain_derive_slopes_dev(self._h, rp, flags, sp), "derive_slopes")

    def read_slopes(self, rect=None):
        """The slope layers the device holds (gbp_terrain_read_slopes_host):
        (dx, dy, dz), each float64 [nx][ny] of rect, the whole map when None."""
        r = L.Rect(0, 0, self.nx, self.ny) if rect is None else L.Rect(*[int(v) for v in rect])
        out = [np.empty((max(r.nx, 0), max(r.ny, 0)), np.float64) for _ in range(3)]
        check(self._lib.gbp_terrain_read_slopes_host(self._h, ctypes.byref(r),
                                                     *[_np_ptr(v) for v in out]), "read_slopes")
        return tuple(out)

    # ---- helpers --------------------------------------------------------------
    def _dev(self, t, dtype, shape_tail=None, name="tensor"):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t))
        t = t.to(device=self.torch_device, dtype=dtype).contiguous()
        if shape_tail is not None:
            t = t.reshape(-1, *shape_tail)
        return t

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.torch_device)

    # ---- K1 -------------------------------------------------------------------
    def height(self, xy):
        xy = self._dev(xy, torch.float64, (2,))
        n = xy.shape[0]
        h = self._empty(n, torch.float64)
        nan = self._empty(n, torch.uint8)
        ood = self._empty(n, torch.uint8)
        check(self._lib.gbp_height_batch_dev(self._h, n, _ptr(xy), _ptr(h), _ptr(nan), _ptr(ood),
                                             _stream(self.device)), "height")
        return h, nan, ood

    def normal(self, xy):
        xy = self._dev(xy, torch.float64, (2,))
        n = xy.shape[0]
        nrm = self._empty((n, 3), torch.float64)
        ood = self._empty(n, torch.uint8)
        check(self._lib.gbp_normal_batch_dev(self._h, n, _ptr(xy), _ptr(nrm), _ptr(ood),
                                             _stream(self.device)), "normal")
        return nrm, ood

    def valid_states(self, states, phase):
        s = self._dev(states, torch.float64, (8,))
        n = s.shape[0]
        ph, pall = (None, int(phase)) if np.ndim(phase) == 0 and not isinstance(phase, torch.Tensor) \
            else (self._dev(phase, torch.uint8), 0)
        v = self._empty(n, torch.uint8)
        f = self._empty(n, torch.int32)
        c = self._empty(n, torch.int32)
        check(self._lib.gbp_valid_states_dev(self._h, n, _ptr(s), _ptr(ph), pall, _ptr(v), _ptr(f),
                                             _ptr(c), _stream(self.device)), "valid_states")
        return v, f, c

    # ---- K2: the hot path -----------------------------------------------------
    def validate_pairs(self, s, a, direction, adaptive=False, s_new=None, t_new=None,
                       out=None):
        """Batched isValidStateActionPair[Reverse] (planning_utils.cpp:645-881).

        `s_new` / `t_new` (optional, device) are in/out like the reference's
        reference parameters: rows the reference would not assign keep their
        contents.  `out` may carry preallocated PairResult buffers (bench)."""
        s = self._dev(s, torch.float64, (8,))
        a = self._dev(a, torch.float64, (10,))
        n = s.shape[0]
        if a.shape[0] != n:
            raise ValueError("s and a batch sizes differ")
        if isinstance(direction, torch.Tensor) or np.ndim(direction) > 0:
            d, dall = self._dev(direction, torch.uint8), 0
        else:
            d, dall = None, int(direction)
        if out is None:
            out = PairResult(
                valid=self._empty(n, torch.uint8),
                s_new=self._dev(s_new, torch.float64, (8,)) if s_new is not None
                else torch.full((n, 8), float("nan"), dtype=torch.float64, device=self.torch_device),
                t_new=self._dev(t_new, torch.float64) if t_new is not None
                else torch.full((n,), float("nan"), dtype=torch.float64, device=self.torch_device),
                flags=self._empty(n, torch.int32),
                counts=self._empty(n, torch.int32))
        check(self._lib.gbp_validate_pairs_dev(
            self._h, n, _ptr(s), _ptr(a), _ptr(d), dall, int(bool(adaptive)), _ptr(out.valid),
            _ptr(out.s_new), _ptr(out.t_new), _ptr(out.flags), _ptr(out.counts),
            _stream(self.device)), "validate_pairs")
        return out

    def validate_pairs_raw(self, n, s_ptr, a_ptr, d_ptr, dall, adaptive, valid_ptr, snew_ptr,
                           tnew_ptr, flags_ptr, counts_ptr, stream_ptr):
        """Pointer-level call for the timed loop (no allocation, no checks)."""
        return self._lib.gbp_validate_pairs_dev(self._h, n, s_ptr, a_ptr, d_ptr, dall, adaptive,
                                                valid_ptr, snew_ptr, tnew_ptr, flags_ptr,
                                                counts_ptr, stream_ptr)

    def shortcut_table(self, paths, adaptive=False):
        """postProcessPath's connect decisions (rrt_connect.cpp:139-227,
        gbp_shortcut_table_dev) for a list of [n_p][8] paths: (reached uint8,
        flags int32), one entry per pair i < j of each path, a path's pairs
        packed row-major over the upper triangle, the paths' consecutive.
        FRAGILE items are left flagged (planner.shortcut_paths re-decides them)."""
        ps = [self._dev(p, torch.float64, (8,)) for p in paths]
        off = np.zeros(len(ps) + 1, np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in ps])
        items = int(sum(p.shape[0] * (p.shape[0] - 1) // 2 for p in ps))
        st = torch.cat(ps) if ps else self._empty((0, 8), torch.float64)
        reached = self._empty(items, torch.uint8)
        flags = self._empty(items, torch.int32)
        check(self._lib.gbp_shortcut_table_dev(self._h, len(ps), _np_ptr(off), _ptr(st),
                                               int(bool(adaptive)), _ptr(reached), _ptr(flags),
                                               _stream(self.device)), "shortcut_table")
        return reached, flags

    # ---- K3 -------------------------------------------------------------------
    def sample_states(self, n, seed, stream_id, index_base=0, require_phase=-1, max_tries=1):
        st = self._empty((n, 8), torch.float64)
        tries = self._empty(n, torch.int32)
        check(self._lib.gbp_sample_states_dev(self._h, n, seed, stream_id, index_base,
                                              int(require_phase), int(max_tries), _ptr(st),
                                              _ptr(tries), _stream(self.device)), "sample_states")
        return st, tries

    def sample_actions(self, normals, seed, stream_id, index_base=0):
        nr = self._dev(normals, torch.float64, (3,))
        n = nr.shape[0]
        a = self._empty((n, 10), torch.float64)
        check(self._lib.gbp_sample_actions_dev(n, _ptr(nr), seed, stream_id, index_base, _ptr(a),
                                               _stream(self.device)), "sample_actions")
        return a

    # ---- direction-biased sampling (gbp_sampling, params.yaml:21-27) --------------
    def set_sampling(self, cfg=None):
        """Install a _lib.Sampling on the handle (None: off); newConfig's candidates
        (extend, extend_host) and the device planner loop's targets use it."""
        check(self._lib.gbp_terrain_set_sampling(self._h, None if cfg is None else ctypes.byref(cfg)),
              "set_sampling")

    def get_sampling(self):
        cfg = L.Sampling()
        check(self._lib.gbp_terrain_get_sampling(self._h, ctypes.byref(cfg)), "get_sampling")
        return cfg

    def sample_states_dir(self, n, seed, stream_id, s_from, s_to, index_base=0, cfg=None):
        """PlannerClass::randomState(terrain, flag, p, speed, s_from, s_to)
        (planner_class.cpp:22-35, :82-148); cfg None: the handle's."""
        st = self._empty((n, 8), torch.float64)
        f = np.ascontiguousarray(s_from, np.float64).reshape(8)
        t = np.ascontiguousarray(s_to, np.float64).reshape(8)
        check(self._lib.gbp_sample_states_dir_dev(
            self._h, n, seed, stream_id, index_base, None if cfg is None else ctypes.byref(cfg),
            _np_ptr(f), _np_ptr(t), _ptr(st), _stream(self.device)), "sample_states_dir")
        return st

    # ---- informed sampling (gbp_informed): targets inside the best cost's ellipse ----
    def set_informed(self, inf=None):
        """Install a _lib.Informed (L.informed_ellipse) on the handle (None: off);
        the device planner loop's targets and the host planner's are drawn in it."""
        check(self._lib.gbp_terrain_set_informed(self._h, None if inf is None else ctypes.byref(inf)),
              "set_informed")

    def get_informed(self):
        inf = L.Informed()
        check(self._lib.gbp_terrain_get_informed(self._h, ctypes.byref(inf)), "get_informed")
        return inf

    def sample_states_informed(self, n, seed, stream_id, s_from=None, s_to=None, index_base=0,
                               cfg=None, inf=None):
        """sample_states_dir's draws with x, y uniform over the ellipse where the
        coin does not pick the direction draw; cfg, inf None: the handle's.
        s_from / s_to are needed only when cfg's state_flag is on."""
        st = self._empty((n, 8), torch.float64)
        f = None if s_from is None else np.ascontiguousarray(s_from, np.float64).reshape(8)
        t = None if s_to is None else np.ascontiguousarray(s_to, np.float64).reshape(8)
        check(self._lib.gbp_sample_states_informed_dev(
            self._h, n, seed, stream_id, index_base, None if cfg is None else ctypes.byref(cfg),
            None if inf is None else ctypes.byref(inf), None if f is None else _np_ptr(f),
            None if t is None else _np_ptr(t), _ptr(st), _stream(self.device)),
            "sample_states_informed")
        return st

    def sample_actions_dir(self, normals, s, s_near, direction, seed, stream_id, index_base=0,
                           cfg=None):
        """getRandomAction(surf_norm, direction, flag, p, s, s_near)
        (planning_utils.cpp:379-391, :443-515); cfg None: the handle's."""
        nr = self._dev(normals, torch.float64, (3,))
        sv = self._dev(s, torch.float64, (8,))
        sn = self._dev(s_near, torch.float64, (8,))
        n = nr.shape[0]
        if isinstance(direction, torch.Tensor) or np.ndim(direction) > 0:
            d, dall = self._dev(direction, torch.uint8), 0
        else:
            d, dall = None, int(direction)
        a = self._empty((n, 10), torch.float64)
        check(self._lib.gbp_sample_actions_dir_dev(
            self._h, n, _ptr(nr), _ptr(sv), _ptr(sn), _ptr(d), dall,
            None if cfg is None else ctypes.byref(cfg), seed, stream_id, index_base, _ptr(a),
            _stream(self.device)), "sample_actions_dir")
        return a

    def extend(self, s_near, target, direction, seed, extend_base=0, adaptive=False):
        """Batched RRTClass::newConfig + extend acceptance (rrt.cpp:20-102)."""
        sn = self._dev(s_near, torch.float64, (8,))
        tg = self._dev(target, torch.float64, (8,))
        n = sn.shape[0]
        if isinstance(direction, torch.Tensor) or np.ndim(direction) > 0:
            d, dall = self._dev(direction, torch.uint8), 0
        else:
            d, dall = None, int(direction)
        r = ExtendResult(
            result=self._empty(n, torch.int32), chosen=self._empty(n, torch.int32),
            s_new=torch.full((n, 8), float("nan"), dtype=torch.float64, device=self.torch_device),
            a_new=torch.full((n, 10), float("nan"), dtype=torch.float64, device=self.torch_device),
            counts=self._empty(n, torch.int32), flags=self._empty(n, torch.int32))
        check(self._lib.gbp_extend_batch_dev(self._h, n, _ptr(sn), _ptr(tg), _ptr(d), dall,
                                             int(bool(adaptive)), seed, extend_base, _ptr(r.result),
                                             _ptr(r.chosen), _ptr(r.s_new), _ptr(r.a_new),
                                             _ptr(r.counts), _ptr(r.flags), _stream(self.device)),
              "extend")
        return r

    # ---- host variants (numpy in/out) -------------------------------------------
    def validate_pairs_host(self, s, a, direction, adaptive=False):
        s = np.ascontiguousarray(s, np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(a, np.float64).reshape(-1, 10)
        n = s.shape[0]
        if np.ndim(direction) > 0:
            d, dall = np.ascontiguousarray(direction, np.uint8), 0
        else:
            d, dall = None, int(direction)
        valid = np.empty(n, np.uint8)
        s_new = np.full((n, 8), np.nan)
        t_new = np.full(n, np.nan)
        flags = np.empty(n, np.uint32)
        counts = np.empty(n, np.uint32)
        check(self._lib.gbp_validate_pairs_host(self._h, n, _np_ptr(s), _np_ptr(a), _np_ptr(d),
                                                dall, int(bool(adaptive)), _np_ptr(valid),
                                                _np_ptr(s_new), _np_ptr(t_new), _np_ptr(flags),
                                                _np_ptr(counts)), "validate_pairs_host")
        return valid, s_new, t_new, flags, counts

    def resolve_fragile(self, s, a, direction, res, adaptive=False):
        """gbp_resolve_fragile_host on a validate_pairs result: numpy copies
        (valid, s_new, t_new, flags, counts) with every GBP_F_FRAGILE attempt
        re-decided on the host with glibc trig; returns them and the number
        re-decided."""
        s = np.ascontiguousarray(_np(s), np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(_np(a), np.float64).reshape(-1, 10)
        n = s.shape[0]
        if np.ndim(direction) > 0 or isinstance(direction, torch.Tensor):
            d, dall = np.ascontiguousarray(_np(direction), np.uint8), 0
        else:
            d, dall = None, int(direction)
        valid = np.ascontiguousarray(_np(res.valid), np.uint8).copy()
        s_new = np.ascontiguousarray(_np(res.s_new), np.float64).copy()
        t_new = np.ascontiguousarray(_np(res.t_new), np.float64).copy()
        flags = np.ascontiguousarray(_np(res.flags)).view(np.uint32).copy()
        counts = np.ascontiguousarray(_np(res.counts)).view(np.uint32).copy()
        k = ctypes.c_int64(0)
        check(self._lib.gbp_resolve_fragile_host(self._h, n, _np_ptr(s), _np_ptr(a), _np_ptr(d),
                                                 dall, int(bool(adaptive)), _np_ptr(valid),
                                                 _np_ptr(s_new), _np_ptr(t_new), _np_ptr(flags),
                                                 _np_ptr(counts), ctypes.byref(k)),
              "resolve_fragile")
        return (valid, s_new, t_new, flags, counts), k.value

    def valid_states_host(self, states, phase):
        """gbp_valid_states_host (FRAGILE states re-decided on the host):
        (valid, flags, counts) numpy."""
        st = np.ascontiguousarray(_np(states), np.float64).reshape(-1, 8)
        n = st.shape[0]
        if np.ndim(phase) > 0:
            ph, pall = np.ascontiguousarray(_np(phase), np.uint8), 0
        else:
            ph, pall = None, int(phase)
        valid = np.empty(n, np.uint8)
        flags = np.empty(n, np.uint32)
        counts = np.empty(n, np.uint32)
        check(self._lib.gbp_valid_states_host(self._h, n, _np_ptr(st), _np_ptr(ph), pall,
                                              _np_ptr(valid), _np_ptr(flags), _np_ptr(counts)),
              "valid_states_host")
        return valid, flags, counts

    def extend_host(self, s_near, target, direction, seed, extend_base=0, adaptive=False):
        """gbp_extend_batch_host (FRAGILE extends re-decided on the host):
        (result, chosen, s_new, a_new, counts, flags) numpy; s_new / a_new NaN
        where the extend is TRAPPED (written only where the reference writes)."""
        sn = np.ascontiguousarray(_np(s_near), np.float64).reshape(-1, 8)
        tg = np.ascontiguousarray(_np(target), np.float64).reshape(-1, 8)
        n = sn.shape[0]
        if np.ndim(direction) > 0 or isinstance(direction, torch.Tensor):
            d, dall = np.ascontiguousarray(_np(direction), np.uint8), 0
        else:
            d, dall = None, int(direction)
        res = np.empty(n, np.int32)
        cho = np.empty(n, np.int32)
        s_new = np.full((n, 8), np.nan)
        a_new = np.full((n, 10), np.nan)
        counts = np.empty(n, np.uint32)
        flags = np.empty(n, np.uint32)
        check(self._lib.gbp_extend_batch_host(self._h, n, _np_ptr(sn), _np_ptr(tg), _np_ptr(d), dall,
                                              int(bool(adaptive)), seed, extend_base, _np_ptr(res),
                                              _np_ptr(cho), _np_ptr(s_new), _np_ptr(a_new),
                                              _np_ptr(counts), _np_ptr(flags)), "extend_host")
        return res, cho, s_new, a_new, counts, flags

    def height_host(self, xy):
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        n = xy.shape[0]
        h = np.empty(n)
        nan = np.empty(n, np.uint8)
        ood = np.empty(n, np.uint8)
        check(self._lib.gbp_height_batch_host(self._h, n, _np_ptr(xy), _np_ptr(h), _np_ptr(nan),
                                              _np_ptr(ood)), "height_host")
        return h, nan, ood


class DeviceTree:
    """A GraphClass / PlannerClass tree resident in HBM (gbp_tree_*): states,
    actions, parents and g on the device, its vertex count too."""

    def __init__(self, root, device=0, capacity=1 << 16):
        self._lib = L.load()
        self.device = int(device)
        h = ctypes.c_void_p()
        check(self._lib.gbp_tree_create(self.device, int(capacity), ctypes.byref(h)), "tree_create")
        self._h = h
        r = np.ascontiguousarray(root, np.float64).reshape(8)
        check(self._lib.gbp_tree_init(self._h, _np_ptr(r), None), "tree_init")

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gbp_tree_destroy(self._h)
            self._h = None

    def __len__(self):
        c = ctypes.c_int64(0)
        check(self._lib.gbp_tree_size(self._h, ctypes.byref(c), None), "tree_size")
        return c.value

    def append(self, states, actions, parents):
        s = np.ascontiguousarray(states, np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(actions, np.float64).reshape(-1, 10)
        p = np.ascontiguousarray(parents, np.int32).reshape(-1)
        check(self._lib.gbp_tree_append_host(self._h, s.shape[0], _np_ptr(s), _np_ptr(a), _np_ptr(p),
                                             None), "tree_append")

    def load(self, states, actions, parents):
        """gbp_tree_load_host: replaces the tree with the given vertices (vertex 0
        the root, parents[0] = -1; parents may follow their children, as RRT*'s
        rewiring leaves them); g is derived on the device from the root down."""
        s = np.ascontiguousarray(states, np.float64).reshape(-1, 8)
        a = np.ascontiguousarray(actions, np.float64).reshape(-1, 10)
        p = np.ascontiguousarray(parents, np.int32).reshape(-1)
        if not s.shape[0] == a.shape[0] == p.shape[0]:
            raise ValueError("states, actions and parents differ in length")
        check(self._lib.gbp_tree_load_host(self._h, s.shape[0], _np_ptr(s), _np_ptr(a), _np_ptr(p),
                                           None), "tree_load")

    def revalidate(self, terrain, direction, adaptive=False, remap_dev=None):
        """gbp_tree_revalidate_host: prunes the tree against `terrain` (an
        engine.Terrain holding the changed map).  A vertex stays when the pair
        check of (v[parent], action, direction) holds on that terrain for every
        edge between it and the root; the root is never tested.  Returns
        (remap, stats): remap [n before] int32, a vertex's new index or -1;
        stats a dict of n_before, n_kept, n_edge_invalid (pruned vertices whose
        own edge failed), n_inherited (pruned through an ancestor only) and
        n_resolved (FRAGILE edges re-decided on the host with glibc).
        remap_dev: an int32 device tensor of at least len(self) elements that
        also receives the remap (gbp_tree_revalidate_keep_host), for
        PlanWorkspace.shared_remap."""
        remap = np.empty(len(self), np.int32)
        st = L.PruneStats()
        k = ctypes.c_int64(0)
        if remap_dev is not None:  # gbp_tree_revalidate_keep_host: the remap stays in HBM too
            check(self._lib.gbp_tree_revalidate_keep_host(terrain._h, self._h, int(direction),
                                                          int(bool(adaptive)), _np_ptr(remap),
                                                          _ptr(remap_dev), remap_dev.numel(),
                                                          ctypes.byref(st), ctypes.byref(k)),
                  "tree_revalidate_keep")
        else:
            check(self._lib.gbp_tree_revalidate_host(terrain._h, self._h, int(direction),
                                                     int(bool(adaptive)), _np_ptr(remap),
                                                     ctypes.byref(st), ctypes.byref(k)),
                  "tree_revalidate")
        stats = {name: getattr(st, name) for name, _ in L.PruneStats._fields_}
        stats["n_resolved"] = k.value
        return remap, stats

    def reroot(self, vertex, terrain=None, direction=L.FORWARD, adaptive=False, remap_dev=None):
        """gbp_tree_reroot_host: makes `vertex` the root and keeps the subtree
        below it, in HBM.  The new root becomes vertex 0 (action zeroed, parent
        -1), the other kept vertices follow in ascending old index, and g is
        derived again from the new root down.  With `terrain` (an
        engine.Terrain holding a changed map) the edges are tested on it as
        revalidate does, and a vertex below the new root stays only when every
        edge between the two holds.  Returns (remap, stats): remap [n before]
        int32, a vertex's new index or -1; stats a dict of n_before, n_kept,
        n_outside (not below the new root), n_edge_invalid, n_inherited (below
        it: own edge failed / an ancestor's did), depth (most edges between
        the new root and a kept vertex) and n_resolved.  remap_dev: as in
        revalidate (gbp_tree_reroot_keep_host)."""
        remap = np.empty(len(self), np.int32)
        st = L.RerootStats()
        k = ctypes.c_int64(0)
        th = terrain._h if terrain is not None else None
        if remap_dev is not None:  # gbp_tree_reroot_keep_host: the remap stays in HBM too
            check(self._lib.gbp_tree_reroot_keep_host(th, self._h, int(vertex), int(direction),
                                                      int(bool(adaptive)), _np_ptr(remap),
                                                      _ptr(remap_dev), remap_dev.numel(),
                                                      ctypes.byref(st), ctypes.byref(k)),
                  "tree_reroot_keep")
        else:
            check(self._lib.gbp_tree_reroot_host(th, self._h, int(vertex), int(direction),
                                                 int(bool(adaptive)), _np_ptr(remap),
                                                 ctypes.byref(st), ctypes.byref(k)), "tree_reroot")
        stats = {name: getattr(st, name) for name, _ in L.RerootStats._fields_}
        stats["n_resolved"] = k.value
        return remap, stats

    def graft(self, root, radius, terrain, direction, adaptive=False, test_edges=False,
              remap_dev=None):
        """gbp_tree_graft_host: makes the state `root`, which need not be a
        vertex, the tree's root, in HBM.  Every vertex within `radius`
        (poseDistance) that `root` connects to directly on `terrain` (depth 0
        of attemptConnect(root, v, direction) is REACHED) becomes a child of the
        new root by that connect action; a vertex stays when such a vertex
        lies on its parent chain (itself included) and, with test_edges, every
        edge up to the nearest one still holds on `terrain`.  The root becomes
        vertex 0, the kept vertices follow in ascending old index, g is
        derived again.  Nothing attached leaves the root alone.  Returns
        (remap, stats): remap [n before] int32; stats a dict of n_before,
        n_kept, n_candidates, n_checked, n_attached, n_outside,
        n_edge_invalid, n_inherited, depth and n_resolved.  remap_dev: as in
        revalidate (gbp_tree_graft_keep_host)."""
        r = np.ascontiguousarray(root, np.float64).reshape(8)
        remap = np.empty(len(self), np.int32)
        st = L.GraftStats()
        k = ctypes.c_int64(0)
        args = (terrain._h, self._h, _np_ptr(r), float(radius), int(direction), int(bool(adaptive)),
                int(bool(test_edges)), _np_ptr(remap))
        if remap_dev is not None:
            check(self._lib.gbp_tree_graft_keep_host(*args, _ptr(remap_dev), remap_dev.numel(),
                                                     ctypes.byref(st), ctypes.byref(k)),
                  "tree_graft_keep")
        else:
            check(self._lib.gbp_tree_graft_host(*args, ctypes.byref(st), ctypes.byref(k)),
                  "tree_graft")
        stats = {name: getattr(st, name) for name, _ in L.GraftStats._fields_}
        stats["n_resolved"] = k.value
        return remap, stats

    def trim(self, other, bound=float("inf"), max_keep=0, protect=-1, remap_dev=None):
        """gbp_tree_trim_host: drops vertices by f = g + poseDistance(v, root of
        `other`), in HBM, on torch's current stream.  A vertex goes when
        f > bound (the held best cost; inf or NaN: no bound) or, with
        1 <= max_keep < len(self), when it is not among the max_keep - 1
        non-root vertices of least f (a group of equal f at the cut goes
        whole); vertex `protect` and its ancestors stay whatever their f
        (-1: none); a vertex below a dropped one goes with it.  The kept
        vertices keep their order and their g, as after revalidate.  Returns
        (remap, stats): remap [n before] int32, a vertex's new index or -1;
        stats a dict of n_before, n_kept, n_over_bound, n_over_budget (not
        over the bound), n_protected (failed a test, kept by protection),
        n_inherited (dropped through an ancestor only), error and cut.
        remap_dev: as in revalidate (gbp_tree_trim_keep_host)."""
        remap = np.empty(len(self), np.int32)
        st = L.TrimStats()
        args = (self._h, other._h, float(bound), int(max_keep), int(protect), _np_ptr(remap))
        if remap_dev is not None:
            check(self._lib.gbp_tree_trim_keep_host(*args, _ptr(remap_dev), remap_dev.numel(),
                                                    ctypes.byref(st), _stream(self.device)),
                  "tree_trim_keep")
        else:
            check(self._lib.gbp_tree_trim_host(*args, ctypes.byref(st), _stream(self.device)),
                  "tree_trim")
        return remap, {name: getattr(st, name) for name, _ in L.TrimStats._fields_}

    def trim_flags(self, other, bound=float("inf"), max_keep=0, protect=-1, n=None):
        """gbp_tree_trim_flags_dev, the trim's stage A, on torch's current
        stream: (keep uint8 [n], f float64 [n], stats int64 [8]) device tensors
        (stats in gbp_trim_stats' layout, its last word the bits of cut); keep
        is what gbp_tree_prune_dev takes as edge_valid."""
        n = len(self) if n is None else int(n)
        dev = torch.device("cuda", self.device)
        keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        f = torch.zeros(n, dtype=torch.float64, device=dev)
        st = torch.zeros(len(L.TrimStats._fields_), dtype=torch.int64, device=dev)
        check(self._lib.gbp_tree_trim_flags_dev(self._h, other._h, n, float(bound), int(max_keep),
                                                int(protect), _ptr(keep), _ptr(f), _ptr(st),
                                                _stream(self.device)), "tree_trim_flags")
        return keep, f, st

    def graft_check(self, root, radius, terrain, direction, adaptive=False):
        """gbp_tree_graft_check_dev, the graft's stage A, on torch's current
        stream: (attach uint8 [n], actions float64 [n, 10], flags int32 [n])
        device tensors.  actions[j] is written where flags[j] has
        F_GRAFT_CHECKED (the rest is zero); a FRAGILE flag is the caller's to
        re-decide."""
        n = len(self)
        dev = terrain.torch_device
        r = np.ascontiguousarray(root, np.float64).reshape(8)
        attach = torch.zeros(n, dtype=torch.uint8, device=dev)
        actions = torch.zeros((n, 10), dtype=torch.float64, device=dev)
        flags = torch.zeros(n, dtype=torch.int32, device=dev)
        check(self._lib.gbp_tree_graft_check_dev(terrain._h, self._h, n, _np_ptr(r), float(radius),
                                                 int(direction), int(bool(adaptive)), _ptr(attach),
                                                 _ptr(actions), _ptr(flags), _stream(self.device)),
              "tree_graft_check")
        return attach, actions, flags

    def graft_apply(self, root, attach, actions, edge_valid=None):
        """gbp_tree_graft_dev, the graft's stage B, under the caller's
        decisions: device tensors attach uint8 [n], actions float64 [n, 10],
        edge_valid uint8 [n] or None.  Returns (remap, stats) as graft does
        (n_candidates = n_checked = 0, no n_resolved)."""
        n = len(self)
        r = np.ascontiguousarray(root, np.float64).reshape(8)
        remap = torch.empty(n, dtype=torch.int32, device=attach.device)
        st = torch.zeros(len(L.GraftStats._fields_), dtype=torch.int64, device=attach.device)
        check(self._lib.gbp_tree_graft_dev(self._h, n, _np_ptr(r), _ptr(attach), _ptr(actions),
                                           _ptr(edge_valid), _ptr(remap), _ptr(st),
                                           _stream(self.device)), "tree_graft_dev")
        names = [name for name, _ in L.GraftStats._fields_]
        return remap.cpu().numpy(), dict(zip(names, st.cpu().tolist()))

    def capacity(self):
        c = ctypes.c_int64(0)
        check(self._lib.gbp_tree_capacity(self._h, ctypes.byref(c)), "tree_capacity")
        return c.value

    def reserve(self, capacity):
        check(self._lib.gbp_tree_reserve(self._h, int(capacity), None), "tree_reserve")

    def read_parents(self):
        """parents [n] int32 alone (4 of a vertex's 156 bytes)."""
        p = np.empty(len(self), np.int32)
        check(self._lib.gbp_tree_read(self._h, 0, p.size, None, None, _np_ptr(p), None, None),
              "tree_read")
        return p

    def read_state(self, i):
        s = np.empty(8)
        check(self._lib.gbp_tree_read(self._h, int(i), 1, _np_ptr(s), None, None, None, None),
              "tree_read")
        return s

    def read(self):
        """(states [n][8], actions [n][10], parents [n], g [n]) numpy."""
        n = len(self)
        s, a = np.empty((n, 8)), np.empty((n, 10))
        p, g = np.empty(n, np.int32), np.empty(n)
        check(self._lib.gbp_tree_read(self._h, 0, n, _np_ptr(s), _np_ptr(a), _np_ptr(p), _np_ptr(g),
                                      None), "tree_read")
        return s, a, p, g


    def read_links(self):
        """(child [n], sibling [n], prev [n]) numpy int32: the successor lists
        (gbp_tree_read_links) — first child, next and previous sibling, -1 none."""
        n = len(self)
        c, s, p = (np.empty(n, np.int32) for _ in range(3))
        check(self._lib.gbp_tree_read_links(self._h, 0, n, _np_ptr(c), _np_ptr(s), _np_ptr(p), None),
              "tree_read_links")
        return c, s, p


class PlanStatus(ctypes.Structure):
    """gbp_plan_status (include/gbp.h)."""
    _fields_ = [("halt", ctypes.c_uint32), ("done", ctypes.c_uint32), ("error", ctypes.c_uint32),
                ("halt_half", ctypes.c_int32), ("n_targets", ctypes.c_int32),
                ("n_validate", ctypes.c_int32), ("n_added", ctypes.c_int32),
                ("added_base", ctypes.c_int32), ("n_conn_added", ctypes.c_int32),
                ("meet_half", ctypes.c_int32), ("meet", ctypes.c_uint64),
                ("ext_base", ctypes.c_int64), ("ext_counter", ctypes.c_int64),
                ("stat_targets", ctypes.c_int64), ("stat_attempts", ctypes.c_int64),
                ("stat_added", ctypes.c_int64), ("stat_conn_added", ctypes.c_int64),
                ("stat_fragile_resolved", ctypes.c_int64), ("stat_depth_capped", ctypes.c_int64),
                ("gate_seq", ctypes.c_uint64), ("stat_nn_rechecks", ctypes.c_int64),
                ("stat_nn_scans", ctypes.c_int64), ("ext_half", ctypes.c_int32),
                ("commit_fin", ctypes.c_uint32), ("ext_prev", ctypes.c_int64),
                ("stat_targets_prev", ctypes.c_int64), ("pre_targets", ctypes.c_int32),
                ("pre_fragile", ctypes.c_int32), ("star_pairs", ctypes.c_int32),
                ("star_rows", ctypes.c_int32), ("n_shared", ctypes.c_int32),
                ("best_a", ctypes.c_int32), ("best_b", ctypes.c_int32), ("star_vrows", ctypes.c_int32),
                ("best_cost", ctypes.c_double), ("stat_star_connects", ctypes.c_int64),
                ("stat_rewires", ctypes.c_int64)]


class PlanWorkspace:
    """Scratch and status of the device planner loop (gbp_plan_ws_*)."""

    def __init__(self, terrain, max_batch):
        self._lib = L.load()
        h = ctypes.c_void_p()
        check(self._lib.gbp_plan_ws_create(terrain._h, int(max_batch), ctypes.byref(h)), "plan_ws")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.gbp_plan_ws_destroy(self._h)
            self._h = None

    def status(self, device=0):
        """gbp_plan_status_read as a dict."""
        st = PlanStatus()
        check(self._lib.gbp_plan_status_read(self._h, ctypes.byref(st), _stream(device)), "status")
        return {k: getattr(st, k) for k, _ in PlanStatus._fields_}

    def reset(self, device=0, extend_counter=0):
        check(self._lib.gbp_plan_reset(self._h, int(extend_counter), _stream(device)), "plan_reset")

    def resolve(self, terrain, tree, other, direction, batch, adaptive=False, device=0):
        """gbp_plan_resolve_host: the halted stage's FRAGILE items re-decided
        with glibc; (stage to resume the halted half at, items re-decided)."""
        resume, nres = ctypes.c_int(-1), ctypes.c_int64(0)
        check(self._lib.gbp_plan_resolve_host(terrain._h, self._h, tree._h, other._h, int(direction),
                                              int(batch), int(bool(adaptive)), ctypes.byref(resume),
                                              ctypes.byref(nres), _stream(device)), "plan_resolve")
        return resume.value, nres.value

    def halves(self, terrain, ta, tb, first_half, n_halves, batch, seed, stream_a=101,
               stream_b=102, adaptive=False, first_stage=0, device=0):
        """gbp_plan_halves_dev: enqueue half-iterations first_half ..
        first_half + n_halves - 1 of the device planner loop (no host sync)."""
        check(self._lib.gbp_plan_halves_dev(terrain._h, self._h, ta._h, tb._h, int(first_half),
                                            int(n_halves), int(batch), int(seed), int(stream_a),
                                            int(stream_b), int(bool(adaptive)), int(first_stage),
                                            _stream(device)), "plan_halves")

    def star_config(self, delta=3.0, max_pairs=1 << 18, max_shared=1 << 22, enable=True):
        """gbp_plan_star_config: RRT*-Connect's insertion stages and its list of
        kept connections (max_shared pairs)."""
        check(self._lib.gbp_plan_star_config(self._h, int(bool(enable)), float(delta), int(max_pairs),
                                             int(max_shared)), "star_config")

    def shared_read(self, max_pairs=None, device=0):
        """gbp_plan_shared_read_host: RRT*'s kept connections in list order and
        the ranked best: (pairs [n][2] int32, best_a, best_b, best_cost)."""
        n = ctypes.c_int64(0)
        ba, bb, bc = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_double(np.inf)
        if max_pairs is None:  # the length first, then the pairs
            check(self._lib.gbp_plan_shared_read_host(self._h, 0, None, ctypes.byref(n), None, None,
                                                      None, _stream(device)), "shared_read")
            max_pairs = n.value
        pairs = np.empty((int(max_pairs), 2), np.int32)
        check(self._lib.gbp_plan_shared_read_host(self._h, pairs.shape[0], _np_ptr(pairs),
                                                  ctypes.byref(n), ctypes.byref(ba), ctypes.byref(bb),
                                                  ctypes.byref(bc), _stream(device)), "shared_read")
        return pairs[:min(n.value, pairs.shape[0])], ba.value, bb.value, bc.value

    def shared_load(self, ta, tb, pairs, device=0):
        """gbp_plan_shared_load_host: replaces the kept connections by `pairs`
        ([n][2], vertices of ta / tb), resets the best and ranks the list with
        the trees' current g.  GbpError E_INVALID_ARG, nothing changed, when an
        index is outside its tree or n exceeds max_shared."""
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        check(self._lib.gbp_plan_shared_load_host(self._h, ta._h, tb._h, p.shape[0], _np_ptr(p),
                                                  _stream(device)), "shared_load")

    def shared_remap(self, ta, tb, remap_a=None, remap_b=None, n_a=None, n_b=None, device=0):
        """gbp_plan_shared_remap_dev: the kept connections through a prune or a
        re-root.  remap_a / remap_b: int32 device tensors as gbp_tree_prune_dev
        / gbp_tree_reroot_dev write them (numpy arrays are uploaded), None =
        that tree did not change (n_* then defaults to its size).  ta / tb are
        the trees after the change.  Returns the stats dict (n_before, n_kept,
        n_dropped_a, n_dropped_b, error), read back after the call."""
        dev = torch.device("cuda", int(device))

        def arg(r, n, tree):
            if r is None:
                return None, (len(tree) if n is None else int(n))
            r = torch.as_tensor(np.ascontiguousarray(r, np.int32) if not isinstance(r, torch.Tensor)
                                else r).to(dev).contiguous()
            if r.dtype != torch.int32:
                raise ValueError("a remap is int32")
            return r, (r.numel() if n is None else int(n))

        ra, na = arg(remap_a, n_a, ta)
        rb, nb = arg(remap_b, n_b, tb)
        st = torch.zeros(5, dtype=torch.int64, device=dev)
        check(self._lib.gbp_plan_shared_remap_dev(self._h, ta._h, tb._h, _ptr(ra), na, _ptr(rb), nb,
                                                  _ptr(st), _stream(device)), "shared_remap")
        vals = st.cpu().tolist()
        return dict(zip((name for name, _ in L.SharedStats._fields_), vals))

    def tree_path(self, ta, tb, ia=-1, ib=-1, max_states=256, device=0):
        """tree_path(ta, tb, ia, ib, ws=self): ia = ib = -1 takes the ranked best."""
        return tree_path(ta, tb, ia, ib, ws=self, max_states=max_states, device=device)

    def nearest(self, tree, queries):
        """gbp_tree_nearest_dev: nearest vertex of `tree` per query (device tensors)."""
        q = queries.contiguous()
        idx = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
        check(self._lib.gbp_tree_nearest_dev(self._h, tree._h, q.shape[0], _ptr(q), _ptr(idx),
                                             _stream(q.device.index or 0)), "tree_nearest")
        return idx

    def extend_tree_host(self, terrain, tree, targets, direction, seed, extend_base=0,
                         adaptive=False):
        """gbp_extend_tree_host: RRTClass::extend (rrt.cpp:77-102) of `tree`
        toward every target, nearest neighbour on the device, successors
        appended in target order: (result, new_vertex, n_resolved)."""
        tg = np.ascontiguousarray(targets, np.float64).reshape(-1, 8)
        n = tg.shape[0]
        res, vtx = np.empty(n, np.int32), np.empty(n, np.int32)
        k = ctypes.c_int64(0)
        check(self._lib.gbp_extend_tree_host(terrain._h, self._h, tree._h, n, _np_ptr(tg),
                                             int(direction), int(bool(adaptive)), seed, extend_base,
                                             _np_ptr(res), _np_ptr(vtx), ctypes.byref(k)),
              "extend_tree_host")
        return res, vtx, k.value


def tree_path(ta, tb, ia, ib, ws=None, max_states=256, device=0, grow=True):
    """gbp_tree_path_host: the joined path of two device trees (ta's root ->
    ia, then tb's ib -> root without ib) without reading the trees:
    (states [n][8], actions [n - 1][10], info), info a dict of n_states,
    n_from_a, n_from_b, error (PATH_E_*), length.  ia = ib = -1 with a
    PlanWorkspace: RRT*'s ranked best (n_states = 0 when there is none).  A
    path longer than max_states reports PATH_E_SHORT and the length needed;
    with `grow` the call is repeated once with that length."""
    lib = L.load()
    while True:
        s, a = np.empty((max(int(max_states), 0), 8)), np.empty((max(int(max_states), 0), 10))
        pi = L.PathInfo()
        check(lib.gbp_tree_path_host(ta._h, int(ia), tb._h, int(ib), ws._h if ws is not None else None,
                                     s.shape[0], _np_ptr(s) if s.size else None,
                                     _np_ptr(a) if a.size else None, ctypes.byref(pi),
                                     _stream(device)), "tree_path")
        info = {k: getattr(pi, k) for k, _ in L.PathInfo._fields_}
        if grow and pi.error == L.PATH_E_SHORT and pi.n_states > s.shape[0]:
            max_states, grow = pi.n_states, False
            continue
        n = 0 if pi.error else pi.n_states
        return s[:n], a[:max(n - 1, 0)], info


def nearest(queries, vertices):
    """Batched PlannerClass::getNearestNeighbor (planner_class.cpp:185-200)."""
    lib = L.load()
    q = queries.contiguous()
    v = vertices.contiguous()
    n = q.shape[0]
    idx = torch.empty(n, dtype=torch.int32, device=q.device)
    dist = torch.empty(n, dtype=torch.float64, device=q.device)
    check(lib.gbp_nearest_batch_dev(n, _ptr(q), v.shape[0], _ptr(v), _ptr(idx), _ptr(dist),
                                    _stream(q.device.index or 0)), "nearest")
    return idx, dist


def neighbors(queries, vertices, radius, max_out=256):
    """Batched PlannerClass::neighborhoodDist (planner_class.cpp:173-182):
    (idx [n, max_out] int32, -1 padded, in the order the reference's vertex map
    iterates keys 0..n_vert-1, gbp_vertex_map_order; count [n])."""
    lib = L.load()
    q = queries.contiguous()
    v = vertices.contiguous()
    n = q.shape[0]
    out = torch.full((n, max_out), -1, dtype=torch.int32, device=q.device)
    cnt = torch.empty(n, dtype=torch.int32, device=q.device)
    check(lib.gbp_neighbors_batch_dev(n, _ptr(q), v.shape[0], _ptr(v), float(radius), max_out,
                                      _ptr(out), _ptr(cnt), _stream(q.device.index or 0)),
          "neighbors")
    return out, cnt


KNN_MAX = 64


def knn(queries, vertices, n_nearest):
    """Batched PlannerClass::neighborhoodN (planner_class.cpp:151-171) on the
    device: (idx [n, n_nearest] int32, dist [n, n_nearest]) in ascending
    (distance, index) order, -1 / NaN past the tree's size; n_nearest <= 64."""
    lib = L.load()
    q = queries.contiguous()
    v = vertices.contiguous()
    n = q.shape[0]
    out = torch.empty((n, int(n_nearest)), dtype=torch.int32, device=q.device)
    dist = torch.empty((n, int(n_nearest)), dtype=torch.float64, device=q.device)
    check(lib.gbp_knn_batch_dev(n, _ptr(q), v.shape[0], _ptr(v), int(n_nearest), _ptr(out),
                                _ptr(dist), _stream(q.device.index or 0)), "knn")
    return out, dist


def knn_yaw(queries, vertices, n_nearest, length_weight=1.0, yaw_weight=1.0):
    """PlannerClass::neighborhoodN with cost_add_yaw set (planner_class.cpp:157-158):
    the key poseDistance * length_weight + stateYawDistance * yaw_weight, the
    yaws formed with glibc on the host (gbp_knn_yaw_batch_host; the scan runs
    on the device).  numpy in, (idx [n, n_nearest] int32, dist) numpy out."""
    lib = L.load()
    q = np.ascontiguousarray(queries, np.float64).reshape(-1, 8)
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 8)
    out = np.empty((q.shape[0], int(n_nearest)), np.int32)
    dist = np.empty((q.shape[0], int(n_nearest)))
    check(lib.gbp_knn_yaw_batch_host(q.shape[0], _np_ptr(q), v.shape[0], _np_ptr(v),
                                     float(length_weight), float(yaw_weight), int(n_nearest),
                                     _np_ptr(out), _np_ptr(dist)), "knn_yaw")
    return out, dist


def device_count():
    lib = L.load()
    c = ctypes.c_int(0)
    lib.gbp_device_count(ctypes.byref(c))
    return c.value
