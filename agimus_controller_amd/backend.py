"""Loader and thin object wrapper of libagimus_hip.so (the product path).

There is no CPU fallback: if the shared library is missing, or no HIP device is
visible, creating a `HipOcp` raises.  The CPU checker under oracle/ is never
imported from here.
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib
import subprocess

import numpy as np

from . import _abi

_CSRC = pathlib.Path(__file__).resolve().parent / "csrc"
LIB_PATH = pathlib.Path(os.environ.get("AGX_LIB", _CSRC / "libagimus_hip.so"))  # AGX_LIB: development override
# The same library with the launch sites of the general-row kernels of large models compiled out (-DAGX_NO_GENERAL_ROWS on the
# unit of the capacities 16 / 30 / 32): built next to the product by the split build, loaded only by the test that compares a
# handle without general rows against it bit for bit (AGX_LIB in a child process).
NOGEN_LIB_PATH = _CSRC / "libagimus_hip_nogen.so"
_LIB = None

# Every symbol include/agimus_hip.h declares (checked by the CPU test-suite).
EXPORTED_SYMBOLS = [
    "agx_last_error", "agx_device_count", "agx_row_nref", "agx_row_nr", "agx_ref_stride",
    "agx_model_create", "agx_model_destroy", "agx_ocp_create", "agx_ocp_destroy", "agx_ocp_set_stream",
    "agx_ocp_sync", "agx_ocp_set_refs", "agx_ocp_set_refs_device", "agx_ocp_solve", "agx_ocp_upload_x0",
    "agx_ocp_upload_warmstart", "agx_ocp_solve_resident", "agx_ocp_download", "agx_ocp_download_first", "agx_ocp_first_packed", "agx_ocp_set_geom_placement", "agx_ocp_reset_duals", "agx_traj_generic_create", "agx_traj_set_horizon_indexes", "agx_ocp_feedback_rollout", "agx_ocp_download_x0", "agx_model_frame_jacobian",
    "agx_ocp_shift_warmstart", "agx_ocp_x0_from_prediction", "agx_ocp_integrate", "agx_model_rnea",
    "agx_model_frame_placement", "agx_ocp_get_residuals", "agx_ocp_calc_diff", "agx_ocp_direction",
    "agx_ocp_time_kernel", "agx_ocp_profile", "agx_traj_sine_create", "agx_traj_set_window",
    "agx_traj_get_point", "agx_traj_warmstart_from_reference", "agx_ocp_mpc_step", "agx_ocp_qp_tiles", "agx_ocp_set_quorum",
    "agx_traj_cartesian_sine_create", "agx_ocp_set_refs_async", "agx_ocp_refs_activate", "agx_ocp_refs_wait", "agx_host_alloc", "agx_host_free",
    "agx_ocp_download_async", "agx_ocp_download_wait",
    "agx_traj_generic_create_weighted", "agx_traj_cartesian_sine_wi_create", "agx_traj_get_tile",
    "agx_ocp_set_plant_inertials", "agx_model_sensitivity", "agx_ocp_cost_wide", "agx_ocp_set_model_inertials",
    "agx_traj_stream_create", "agx_traj_stream_append", "agx_traj_stream_release", "agx_traj_stream_range",
    "agx_traj_stream_joins", "agx_traj_stream_timing", "agx_ocp_set_obstacle_placements",
    "agx_ocp_set_first_pack", "agx_ocp_first_pack_counts", "agx_ocp_handoff_counts",
    "agx_ocp_iter_log", "agx_ocp_iter_log_read", "agx_ocp_item_costs", "agx_ocp_carry_counts", "agx_ocp_general_rows",
    "agx_ocp_clearance", "agx_ocp_last_direction", "agx_ocp_set_step_tail",
]  # fmt: skip


def _run(cmd, verbose):
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError(f"{cmd[0]} failed ({res.returncode}): {res.stderr[-2000:]}")


def build(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU).

    The kernels are templates over the model size; one translation unit with every size takes ~6
    minutes on one core, so the source is compiled once per group of sizes (csrc/agx_front.py: GROUPS)
    in parallel processes -- namespace and entry points suffixed per group -- and linked with a
    generated front that forwards each call to the group owning the handle.  AGX_BUILD_SPLIT=0 builds
    the single translation unit instead."""
    hdr = _CSRC.parent.parent / "include" / "agimus_hip.h"
    pairs_src = _CSRC / "agx_cost_pairs.hip"  # the wide-cost-set kernels: a translation unit of their own (see the file)
    diag_src = _CSRC / "agx_diag.hip"  # the diagnostics kernels (iteration log, per-item costs): likewise, one unit for every capacity
    gen_src = _CSRC / "agx_general_rows.hip"  # the general cost rows of large models: likewise, the capacities of group 1
    srcs = [_CSRC / "agimus_hip.hip"] + sorted(_CSRC.glob("*.hpp")) + [hdr, _CSRC / "agx_front.py", pairs_src, diag_src, gen_src]
    split = os.environ.get("AGX_BUILD_SPLIT", "1") != "0"
    newest = max(s.stat().st_mtime for s in srcs)
    if not force and all(p.exists() and p.stat().st_mtime >= newest for p in ([LIB_PATH, NOGEN_LIB_PATH] if split else [LIB_PATH])):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
    if not split:
        _run(base + [f"-I{hdr.parent}", "-shared", "-o", str(LIB_PATH), str(srcs[0]), str(pairs_src), str(diag_src), str(gen_src)], verbose)
        return LIB_PATH
    import importlib.util

    spec = importlib.util.spec_from_file_location("agx_front", _CSRC / "agx_front.py")
    front = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(front)
    obj = _CSRC.parent.parent / "build" / "obj"
    obj.mkdir(parents=True, exist_ok=True)
    names = [n for _, n, _ in front.prototypes(hdr.read_text())]
    procs = []
    for g in front.GROUPS:
        cmd = base + ["-c", f"-I{hdr.parent}"] + front.rename_flags(names, g) + ["-o", str(obj / f"agx_g{g}.o"), str(srcs[0])]
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    g1 = max(front.GROUPS)  # the unit of the large capacities once more, without the launch sites of the general-row kernels
    cmd = base + ["-c", f"-I{hdr.parent}", "-DAGX_NO_GENERAL_ROWS"] + front.rename_flags(names, g1) + ["-o", str(obj / f"agx_g{g1}_nogen.o"), str(srcs[0])]
    procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    cmd = base + ["-c", f"-I{hdr.parent}", "-DAGX_GROUP=0", "-o", str(obj / "agx_cost_pairs.o"), str(pairs_src)]  # the sizes of group 0
    procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    cmd = base + ["-c", f"-I{hdr.parent}", "-o", str(obj / "agx_diag.o"), str(diag_src)]
    procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    cmd = base + ["-c", f"-I{hdr.parent}", "-DAGX_GROUP=1", "-o", str(obj / "agx_general_rows.o"), str(gen_src)]  # the sizes of group 1
    procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    (obj / "agx_front.cpp").write_text(front.front_source(hdr.read_text()))
    _run(["g++", "-O2", "-std=c++17", "-fPIC", f"-I{hdr.parent}", "-c", "-o", str(obj / "agx_front.o"), str(obj / "agx_front.cpp")], verbose)
    failed = None
    for cmd, p in procs:
        out, err = p.communicate()
        if verbose or p.returncode != 0:
            print(out, err)
        if p.returncode != 0 and failed is None:
            failed = RuntimeError(f"hipcc failed ({p.returncode}) for {cmd[-1]} [{cmd[-3]}]: {err[-2000:]}")
    if failed:
        raise failed
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB_PATH)] + [str(obj / f"agx_g{g}.o") for g in front.GROUPS]
         + [str(obj / "agx_cost_pairs.o"), str(obj / "agx_diag.o"), str(obj / "agx_general_rows.o"), str(obj / "agx_front.o")], verbose)
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(NOGEN_LIB_PATH)]
         + [str(obj / (f"agx_g{g}_nogen.o" if g == g1 else f"agx_g{g}.o")) for g in front.GROUPS]
         + [str(obj / "agx_cost_pairs.o"), str(obj / "agx_diag.o"), str(obj / "agx_general_rows.o"), str(obj / "agx_front.o")], verbose)
    return LIB_PATH


def lib():
    """The loaded library; raises if it has not been built."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP path has no CPU fallback)"
            )
        _LIB = C.CDLL(str(LIB_PATH))
        _LIB.agx_last_error.restype = C.c_char_p
    return _LIB


def device_count() -> int:
    return int(lib().agx_device_count())


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f8(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        assert a.shape == tuple(shape), f"expected shape {tuple(shape)}, got {a.shape}"
    return a


class HipError(RuntimeError):
    pass


class _PinnedBlock:
    """Owner of one page-locked allocation (agx_host_alloc); freed with the last array that views it."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        lib().agx_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        if lib().agx_host_alloc(C.c_size_t(nbytes), C.byref(self.ptr)) != 0:
            raise HipError(lib().agx_last_error().decode())
        self.buf = (C.c_char * nbytes).from_address(self.ptr.value)

    def __del__(self):
        try:
            lib().agx_host_free.argtypes = [C.c_void_p]
            lib().agx_host_free(self.ptr)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def pinned_array(shape, dtype=np.float64) -> np.ndarray:
    """numpy array over page-locked host memory: transfers to and from it run at the rate of the link and asynchronously."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    block = _PinnedBlock(max(n * dtype.itemsize, 1))
    arr = np.frombuffer(block.buf, dtype=dtype, count=n).reshape(shape)
    arr.flags.writeable = True
    _PINNED[id(block)] = block  # np.frombuffer keeps block.buf alive, not the block: tie the block's life to the array's
    import weakref

    weakref.finalize(arr.base if arr.base is not None else arr, _PINNED.pop, id(block), None)
    return arr


_PINNED: dict = {}


def _chk(rc):
    if rc != 0:
        raise HipError(lib().agx_last_error().decode())


class HipOcp:
    """Device-resident batch of B shooting problems sharing one model and cost table."""

    def __init__(self, table, packed_ocp: _abi.PackedOcp, batch: int = 1, device: int = 0):
        L = lib()
        self.table = table
        self.pm = _abi.PackedModel(table)
        self.po = packed_ocp
        self.nv = self.pm.nv
        self.nx, self.nu = 2 * self.nv, self.nv
        self.T, self.B = packed_ocp.horizon, int(batch)
        self.stride = packed_ocp.stride
        self.tile = _abi.tile_doubles(self.nv)
        self._log_cap = 0  # capacity of the per-iteration solver log (iter_log); 0: off
        self._m = C.c_void_p()
        self._h = C.c_void_p()
        _chk(L.agx_model_create(C.byref(self.pm.desc), C.byref(self._m)))
        rc = L.agx_ocp_create(self._m, C.byref(self.po.desc), self.B, int(device), C.byref(self._h))
        if rc != 0:
            msg = L.agx_last_error().decode()
            L.agx_model_destroy(self._m)
            self._m = None
            raise HipError(msg)

    @property
    def cost_wide(self) -> bool:
        """The handle runs a wide cost set (agx_ocp_cost_wide): set_refs then takes no frame-id table."""
        return lib().agx_ocp_cost_wide(self._h) == 1

    @property
    def general_rows(self) -> bool:
        """The handle has an active ControlGrav / FrameVelocity cost row (agx_ocp_general_rows): the kernels that carry Lxu and
        the dense Lxx blocks run."""
        return lib().agx_ocp_general_rows(self._h) == 1

    def close(self):
        if getattr(self, "_h", None):
            lib().agx_ocp_destroy(self._h)
            self._h = None
        if getattr(self, "_m", None):
            lib().agx_model_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- references ---------------------------------------------------------
    def set_refs(self, ref_tile, frames=None):
        ref = _f8(ref_tile, (self.B, self.T + 1, self.stride))
        fr = None
        if frames is not None:
            fr = np.ascontiguousarray(frames, dtype=np.int32)
            assert fr.shape == (self.B, self.T + 1, _abi.AGX_MAX_ROWS)
        _chk(lib().agx_ocp_set_refs(self._h, _p(ref), _p(fr)))

    def set_refs_async(self, ref_tile, frames=None):
        """Stages a tile (ideally a `pinned_array`): a second stream copies it while the solver still works on the current one;
        refs_activate() swaps it in.  Keep the buffer untouched until the solve after its activation has returned."""
        ref = np.asarray(ref_tile)
        assert ref.dtype == np.float64 and ref.flags.c_contiguous and ref.shape == (self.B, self.T + 1, self.stride)
        fr = None
        if frames is not None:
            fr = np.asarray(frames)
            assert fr.dtype == np.int32 and fr.flags.c_contiguous and fr.shape == (self.B, self.T + 1, _abi.AGX_MAX_ROWS)
        self._async_keep = (ref, fr)  # the copy reads the buffers after this call returns
        _chk(lib().agx_ocp_set_refs_async(self._h, _p(ref), _p(fr)))

    def refs_wait(self):
        _chk(lib().agx_ocp_refs_wait(self._h))

    def refs_activate(self):
        """The tile staged by set_refs_async becomes the current one (device-side wait, no host stall)."""
        _chk(lib().agx_ocp_refs_activate(self._h))

    def download_async(self, xs=None, us=None, K=None):
        """Full results into caller-owned arrays (ideally `pinned_array`s) behind the solver's back: complete after download_wait()."""
        for a, shape in ((xs, (self.B, self.T + 1, self.nx)), (us, (self.B, self.T, self.nu)), (K, (self.B, self.T, self.nu, self.nx))):
            assert a is None or (a.dtype == np.float64 and a.flags.c_contiguous and a.shape == shape)
        self._dl_keep = (xs, us, K)
        _chk(lib().agx_ocp_download_async(self._h, _p(xs), _p(us), _p(K)))

    def download_wait(self):
        _chk(lib().agx_ocp_download_wait(self._h))

    def set_stream(self, raw_stream: int):
        _chk(lib().agx_ocp_set_stream(self._h, C.c_void_p(raw_stream)))

    def sync(self):
        _chk(lib().agx_ocp_sync(self._h))

    # -- solve --------------------------------------------------------------
    def solve(self, x0, xs_ws, us_ws, max_iter, max_time=0.0):
        x0 = _f8(x0, (self.B, self.nx))
        xs_ws = _f8(xs_ws, (self.B, self.T + 1, self.nx))
        us_ws = _f8(us_ws, (self.B, self.T, self.nu))
        xs = np.empty_like(xs_ws)
        us = np.empty_like(us_ws)
        K = np.empty((self.B, self.T, self.nu, self.nx))
        st = np.zeros(self.B, dtype=_abi.STATUS_DTYPE)
        _chk(lib().agx_ocp_solve(self._h, _p(x0), _p(xs_ws), _p(us_ws), int(max_iter), C.c_double(max_time),
                                 _p(xs), _p(us), _p(K), _p(st)))  # fmt: skip
        return xs, us, K, st

    def upload_x0(self, x0):
        _chk(lib().agx_ocp_upload_x0(self._h, _p(_f8(x0, (self.B, self.nx)))))

    def upload_warmstart(self, xs, us):
        xs = _f8(xs, (self.B, self.T + 1, self.nx))
        us = _f8(us, (self.B, self.T, self.nu))
        _chk(lib().agx_ocp_upload_warmstart(self._h, _p(xs), _p(us)))

    def solve_resident(self, max_iter, max_time=0.0):
        _chk(lib().agx_ocp_solve_resident(self._h, int(max_iter), C.c_double(max_time)))

    def download(self, want_K=True):
        xs = np.empty((self.B, self.T + 1, self.nx))
        us = np.empty((self.B, self.T, self.nu))
        K = np.empty((self.B, self.T, self.nu, self.nx)) if want_K else None
        st = np.zeros(self.B, dtype=_abi.STATUS_DTYPE)
        _chk(lib().agx_ocp_download(self._h, _p(xs), _p(us), _p(K), _p(st)))
        return xs, us, K, st

    def download_first(self, want_status=True, copy=True):
        """us[0], K[0], xs[1] (+ status) of every instance out of the handle's pinned buffer.  Instances that converge write
        their record into it during the solve; when all of them did, this call launches and waits for nothing, otherwise one
        pack kernel fills the buffer.  copy=False returns views into that buffer, valid until the next call that solves
        (solve, solve_resident, mpc_step) or packs (download_first)."""
        ptr = C.POINTER(C.c_double)()
        stride = C.c_int(0)
        _chk(lib().agx_ocp_first_packed(self._h, C.byref(ptr), C.byref(stride)))
        addr = C.addressof(ptr.contents)
        cached = getattr(self, "_first_view", None)
        if cached is None or cached[0] != addr:
            cached = (addr, np.ctypeslib.as_array(ptr, shape=(self.B, stride.value)))
            self._first_view = cached  # the pinned buffer lives as long as the handle
        buf = cached[1]
        nu, nx = self.nu, self.nx
        nk = nu * nx
        us0 = buf[:, :nu]
        K0 = buf[:, nu:nu + nk].reshape(self.B, nu, nx)
        x1 = buf[:, nu + nk:nu + nk + nx]
        if copy:
            us0, K0, x1 = us0.copy(), K0.copy(), x1.copy()
        st = None
        if want_status:
            q = buf[:, nu + nk + nx:]
            names = ("kkt", "cost", "merit", "gap_norm", "iter", "qp_iters", "solved", "flags")
            if copy:
                st = np.zeros(self.B, dtype=_abi.STATUS_DTYPE)
                for k, name in enumerate(names):
                    st[name] = q[:, k] if k < 4 else q[:, k].astype(np.int32)
            else:
                st = {name: q[:, k] for k, name in enumerate(names)}  # views (float64) into the pinned buffer
        return us0, K0, x1, st

    def set_first_pack(self, in_solve: bool = True):
        """False: no first-node record is written during a solve; download_first always packs with a launch of its own."""
        _chk(lib().agx_ocp_set_first_pack(self._h, 1 if in_solve else 0))

    def first_pack_counts(self):
        """(download_first calls served from records written during the solve, calls served by the pack kernel)."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        _chk(lib().agx_ocp_first_pack_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def handoff_counts(self):
        """(solves that ended on the hand-off right behind the head of the step, instances whose tiles the next mpc_step may
        inherit as the last solve published it)."""
        a, b = C.c_longlong(0), C.c_int(0)
        _chk(lib().agx_ocp_handoff_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def carry_counts(self):
        """(mpc_step calls whose first derivative pass inherited the previous step's tiles, calls that ran the full pass)."""
        a, b = C.c_longlong(0), C.c_longlong(0)
        _chk(lib().agx_ocp_carry_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_geom_placement(self, frame: int, se3_12):
        """OCPBaseCroco.update_geometry_placement (ocp_base_croco.py:110-132) for a geometry frame."""
        _chk(lib().agx_ocp_set_geom_placement(self._h, int(frame), _p(_f8(se3_12).reshape(12))))

    def set_quorum(self, sqp_fraction: float = 1.0, qp_fraction: float = 1.0):
        """Batch policy: end the SQP / ADMM loops once this fraction of the instances has finished (see agimus_hip.h)."""
        _chk(lib().agx_ocp_set_quorum(self._h, C.c_double(sqp_fraction), C.c_double(qp_fraction)))

    def reset_duals(self):
        _chk(lib().agx_ocp_reset_duals(self._h))

    def shift_warmstart(self):
        _chk(lib().agx_ocp_shift_warmstart(self._h))

    def x0_from_prediction(self):
        _chk(lib().agx_ocp_x0_from_prediction(self._h))

    def integrate(self, x, u):
        x = _f8(x).reshape(-1, self.nx)
        u = _f8(u).reshape(-1, self.nu)
        out = np.empty_like(x)
        _chk(lib().agx_ocp_integrate(self._h, x.shape[0], _p(x), _p(u), _p(out)))
        return out

    def rnea(self, q, v, a):
        q = _f8(q).reshape(-1, self.nv)
        v = _f8(v).reshape(-1, self.nv)
        a = _f8(a).reshape(-1, self.nv)
        tau = np.empty_like(q)
        _chk(lib().agx_model_rnea(self._h, q.shape[0], _p(q), _p(v), _p(a), _p(tau)))
        return tau

    def frame_placement(self, frame: int, q):
        q = _f8(q).reshape(-1, self.nv)
        out = np.empty((q.shape[0], 12))
        _chk(lib().agx_model_frame_placement(self._h, q.shape[0], int(frame), _p(q), _p(out)))
        return out

    def frame_jacobian(self, frame: int, q, local: bool = False):
        """pinocchio.getFrameJacobian: [n, 6, nv], rows linear | angular; LOCAL_WORLD_ALIGNED or LOCAL."""
        q = _f8(q).reshape(-1, self.nv)
        J = np.empty((q.shape[0], 6, self.nv))
        _chk(lib().agx_model_frame_jacobian(self._h, q.shape[0], int(frame), 1 if local else 0, _p(q), _p(J)))
        return J

    def residuals(self, row: int):
        nr = _abi.row_nr(self.po.running[row].kind, self.nv)
        out = np.empty((self.B, self.T, nr))
        _chk(lib().agx_ocp_get_residuals(self._h, int(row), _p(out)))
        return out

    # -- diagnostics --------------------------------------------------------
    def iter_log(self, capacity: int):
        """Per-iteration solver log (agx_ocp_iter_log): room for `capacity` records per instance; 0 switches it off.  While on,
        every solve / solve_resident / mpc_step starts the log afresh; results are the same with the log on or off."""
        _chk(lib().agx_ocp_iter_log(self._h, int(capacity)))
        self._log_cap = int(capacity)

    def read_iter_log(self):
        """(records, n): records [B][capacity] structured array (_abi.ITER_RECORD_DTYPE, record j = SQP iteration j), n [B] the
        iterations every instance started in the last solve (records at or beyond the capacity are dropped, n still counts
        them).  `solver_log.SolverLog.from_records` turns the pair into arrays per field and a table."""
        cap = self._log_cap
        if cap <= 0:
            raise HipError("read_iter_log: the log is off (iter_log(capacity))")
        rec = np.zeros((self.B, cap), dtype=_abi.ITER_RECORD_DTYPE)
        n = np.zeros(self.B, dtype=np.int32)
        _chk(lib().agx_ocp_iter_log_read(self._h, _p(rec), _p(n)))
        return rec, n

    def item_costs(self):
        """Every cost item of every node on its own at the resident (xs, us) (agx_ocp_item_costs): a dict with
        cost_r [B][T][Rr], Lx_r [B][T][Rr][nx], Lu_r [B][T][Rr][nu], cost_t [B][Rt], Lx_t [B][Rt][nx]; Rr / Rt: all rows of the
        running / terminal table.  Differential level: item weight x activation, WITHOUT the factor dt of a running node.  The
        call only reads (iterate, solver state and tile carry are untouched)."""
        Rr, Rt = len(self.po.running), len(self.po.terminal)
        out = {"cost_r": np.empty((self.B, self.T, Rr)), "Lx_r": np.empty((self.B, self.T, Rr, self.nx)),
               "Lu_r": np.empty((self.B, self.T, Rr, self.nu)), "cost_t": np.empty((self.B, Rt)), "Lx_t": np.empty((self.B, Rt, self.nx))}  # fmt: skip
        _chk(lib().agx_ocp_item_costs(self._h, _p(out["cost_r"]), _p(out["Lx_r"]), _p(out["Lu_r"]), _p(out["cost_t"]), _p(out["Lx_t"])))
        return out

    def clearance(self, pairs, q=None, witness=False, minimum=False):
        """Signed distances of the geometry pairs `pairs` (agx_ocp_clearance): a sequence of (frame_a, frame_b), frame ids or names of
        the table -- any pairs, rows of the problem or not.  q [B, m, nv]: the configurations; None: the resident iterate, m = T + 1
        samples, terminal node included.  Returns dist [B, m, n]; with witness=True also [B, m, n, 3, 3] (point on a, point on b,
        unit normal n, world frame, the points on the surfaces: pa - pb = dist n); with minimum=True also (min_dist [B],
        min_where [B, 2]: sample and pair, the first of equal ones).  In that order, as a tuple when more than dist is asked for.
        World-fixed frames stand where the solve sees them (set_geom_placement, set_obstacle_placements).  The call only reads."""
        names = self.table.frame_names

        def frame(f):
            if isinstance(f, str):
                if f not in names:
                    raise ValueError(f"pairs: the table has no frame {f!r}")
                return names.index(f)
            return int(f)

        try:
            ids = [[frame(f) for f in pair] for pair in pairs]
        except TypeError:
            raise ValueError("pairs: expected a sequence of (frame_a, frame_b)") from None
        n = len(ids)
        if n < 1 or any(len(pair) != 2 for pair in ids):
            raise ValueError("pairs: expected at least one (frame_a, frame_b)")
        fr = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).T)
        if q is None:
            m = self.T + 1
        else:
            q = np.ascontiguousarray(np.asarray(q, dtype=np.float64))
            if q.ndim != 3 or q.shape[0] != self.B or q.shape[1] < 1 or q.shape[2] != self.nv:
                raise ValueError(f"q: expected shape ({self.B}, m, {self.nv}) with m >= 1, got {q.shape}")
            m = q.shape[1]
        dist = np.empty((self.B, m, n))
        wit = np.empty((self.B, m, n, 3, 3)) if witness else None
        dmin = np.empty(self.B) if minimum else None
        where = np.empty((self.B, 2), dtype=np.int32) if minimum else None
        _chk(lib().agx_ocp_clearance(self._h, C.c_int(n), _p(fr[0]), _p(fr[1]), _p(q), C.c_int(m), _p(dist), _p(wit), _p(dmin), _p(where)))
        out = (dist,) + ((wit,) if witness else ()) + (((dmin, where),) if minimum else ())
        return out[0] if len(out) == 1 else out

    # -- kernel level -------------------------------------------------------
    def calc_diff(self, want_tiles=True):
        tiles = np.empty((self.B, self.T + 1, self.tile)) if want_tiles else None
        _chk(lib().agx_ocp_calc_diff(self._h, _p(tiles)))
        return tiles

    def qp_tiles(self):
        """QP tile and aux tile of every node at the resident point: dicts of blocks (see agx_ocp_qp_tiles)."""
        qs, as_ = C.c_int(0), C.c_int(0)
        _chk(lib().agx_ocp_qp_tiles(self._h, None, None, C.byref(qs), C.byref(as_)))
        qt = np.empty((self.B, self.T + 1, qs.value))
        aux = np.empty((self.B, self.T + 1, as_.value))
        _chk(lib().agx_ocp_qp_tiles(self._h, _p(qt), _p(aux), C.byref(qs), C.byref(as_)))
        # the tiles are laid out at the handle's capacity NV >= nv (a model below a capacity is padded with joints at the end)
        nv, ld = self.nv, (8 if (qs.value - 48) % 48 == 0 and (qs.value - 48) // 48 <= 8 else 32)
        NV = (qs.value - 5 * ld - 8) // (6 * ld)
        assert NV >= nv and qs.value == 6 * NV * ld + 5 * ld + 8 and as_.value == 4 * NV * ld + 3 * ld, (nv, qs.value, as_.value)
        b2 = NV * ld
        blk = lambda a, off: a[..., off:off + b2].reshape(self.B, self.T + 1, NV, ld)[..., :nv, :nv]  # noqa: E731
        pair = lambda a, off: np.concatenate([a[..., off:off + nv], a[..., off + NV:off + NV + nv]], axis=-1)  # noqa: E731
        q = {name: blk(qt, k * b2) for k, name in enumerate(("Hqq", "Hqv", "Hvv", "Hqw", "Hvw", "Hww"))}
        o = 6 * b2
        q["gx"] = pair(qt, o)
        q["gw"] = qt[..., o + 2 * ld:o + 2 * ld + nv]
        q["f"] = pair(qt, o + 3 * ld)
        q["cost"] = qt[..., o + 5 * ld]
        a = {name: blk(aux, k * b2) for k, name in enumerate(("M", "tq", "tv", "Lqq"))}
        o = 4 * b2
        a["Lvv"], a["Luu"], a["Lu"] = aux[..., o:o + nv], aux[..., o + ld:o + ld + nv], aux[..., o + 2 * ld:o + 2 * ld + nv]
        return q, a

    def direction(self):
        K = np.empty((self.B, self.T, self.nu, self.nx))
        k = np.empty((self.B, self.T, self.nu))
        dx = np.empty((self.B, self.T + 1, self.nx))
        du = np.empty((self.B, self.T, self.nu))
        kkt = np.empty(self.B)
        _chk(lib().agx_ocp_direction(self._h, _p(K), _p(k), _p(dx), _p(du), _p(kkt)))
        return K, k, dx, du, kkt

    def set_step_tail(self, on: bool = True):
        """k_step_tail (default) or forward pass, node KKT pass and head of the step as three launches; from the next solve on."""
        _chk(lib().agx_ocp_set_step_tail(self._h, int(bool(on)), None))

    def step_tail_launches(self) -> int:
        """k_step_tail launches of this handle so far (0: its solves ran forward pass, node KKT pass and head as three launches)."""
        n = C.c_longlong(0)
        _chk(lib().agx_ocp_set_step_tail(self._h, -1, C.byref(n)))
        return int(n.value)

    def last_direction(self):
        """dx, du and the node shares {kkt, cost, gap, violation} as the last SQP iteration of the last solve left them."""
        dx = np.empty((self.B, self.T + 1, self.nx))
        du = np.empty((self.B, self.T, self.nu))
        nodestat = np.empty((self.B, self.T + 1, 4))
        _chk(lib().agx_ocp_last_direction(self._h, _p(dx), _p(du), _p(nodestat)))
        return dx, du, nodestat

    def time_kernel(self, which: int, reps: int) -> float:
        ms = C.c_double()
        _chk(lib().agx_ocp_time_kernel(self._h, int(which), int(reps), C.byref(ms)))
        return ms.value

    def profile(self, enable: bool):
        """Switch in-situ kernel timing on/off; returns (ms_sum[3], count[3]) accumulated so far."""
        ms = (C.c_double * 3)()
        cnt = (C.c_longlong * 3)()
        _chk(lib().agx_ocp_profile(self._h, 1 if enable else 0, ms, cnt))
        return list(ms), list(cnt)

    # -- resident trajectory -------------------------------------------------
    def sine_trajectory(self, n_points, dt, q0, amp, pulsation, scale_duration, t0, w_q, w_qdot, w_effort, w_pose, frame):
        B, nv = self.B, self.nv
        bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        args = [bc(q0, (B, nv)), bc(amp, (B, nv)), bc(pulsation, (B, nv)), bc(scale_duration, (B, nv)), bc(t0, (B,)),
                bc(w_q, (nv,)), bc(w_qdot, (nv,)), bc(w_effort, (nv,)), bc(w_pose, (6,))]  # fmt: skip
        _chk(lib().agx_traj_sine_create(self._h, int(n_points), C.c_double(dt), *[_p(a) for a in args], int(frame)))

    def generic_trajectory(self, q, dq, ddq, w_q, w_qdot, w_effort, w_pose, frame):
        """Resident trajectory from samples q, dq, ddq [B][n_points][nv] (GenericTrajectory upstream)."""
        B, nv = self.B, self.nv
        q, dq, ddq = (_f8(a).reshape(B, -1, nv) for a in (q, dq, ddq))
        assert q.shape == dq.shape == ddq.shape
        bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        _chk(lib().agx_traj_generic_create(self._h, int(q.shape[1]), _p(q), _p(dq), _p(ddq), _p(bc(w_q, (nv,))), _p(bc(w_qdot, (nv,))),
                                           _p(bc(w_effort, (nv,))), _p(bc(w_pose, (6,))), int(frame)))

    def cartesian_sine_trajectory(self, n_points, dt, q0, amp, pulsation, w_q, w_qdot, w_effort, w_pose, frame,
                                  scale_duration=0.2, precision=1e-5, it_max=10000):
        """Resident trajectory of the Cartesian sine generator (SinusWaveCartesianSpace upstream): inverse kinematics of
        every instance and point on the device.  q0 [B][nv], amp / pulsation [B][3]."""
        B, nv = self.B, self.nv
        bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        _chk(lib().agx_traj_cartesian_sine_create(self._h, int(n_points), C.c_double(dt), _p(bc(q0, (B, nv))), _p(bc(amp, (B, 3))),
                                                  _p(bc(pulsation, (B, 3))), C.c_double(scale_duration), C.c_double(precision), int(it_max),
                                                  _p(bc(w_q, (nv,))), _p(bc(w_qdot, (nv,))), _p(bc(w_effort, (nv,))), _p(bc(w_pose, (6,))),
                                                  int(frame)))

    def generic_trajectory_weighted(self, q, dq, ddq, w_q, w_qdot, w_effort, w_pose, frame, pose=None, w_collision=None):
        """Resident trajectory from samples q, dq, ddq [B][n_points][nv] with a weight schedule (GenericVisualServoingTrajectory
        upstream; `schedule_arrays` of that class gives the three arrays): w_pose [n_points][6] pose weights, pose [n_points][12]
        end-effector references instead of the forward kinematics of q, w_collision [n_points] item weight of the collision
        rows.  The per-sample arrays broadcast over B."""
        B, nv = self.B, self.nv
        q, dq, ddq = (_f8(a).reshape(B, -1, nv) for a in (q, dq, ddq))
        assert q.shape == dq.shape == ddq.shape
        n = q.shape[1]
        bc = lambda a, shape: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        _chk(lib().agx_traj_generic_create_weighted(self._h, int(n), _p(q), _p(dq), _p(ddq), _p(bc(w_q, (nv,))), _p(bc(w_qdot, (nv,))),
                                                    _p(bc(w_effort, (nv,))), int(frame), _p(bc(pose, (B, n, 12))), _p(bc(w_pose, (B, n, 6))),
                                                    _p(bc(w_collision, (B, n)))))

    def cartesian_sine_weight_increasing_trajectory(self, n_points, dt, q0, amp, pulsation, period, w_increasing, w_q, w_qdot, w_effort,
                                                    w_pose, frame, scale_duration=0.2, precision=1e-5, it_max=10000):
        """Resident trajectory of SinusWaveCartesianSpaceWeightIncreasing upstream: the joints follow the Cartesian sine, the
        end-effector target switches between its extrema and the translational pose weight ramps over every half cycle.
        q0 [B][nv], amp / pulsation / period [B][3]; `w_increasing`: a trajectories.weight_increasing.WeightIncreasing; the last
        three entries of w_pose are the rotational weights."""
        B, nv = self.B, self.nv
        bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        rate = float(np.arctanh(w_increasing.percent) / w_increasing.time_reach_percent)
        _chk(lib().agx_traj_cartesian_sine_wi_create(self._h, int(n_points), C.c_double(dt), _p(bc(q0, (B, nv))), _p(bc(amp, (B, 3))),
                                                     _p(bc(pulsation, (B, 3))), C.c_double(scale_duration), C.c_double(precision), int(it_max),
                                                     _p(bc(w_q, (nv,))), _p(bc(w_qdot, (nv,))), _p(bc(w_effort, (nv,))), _p(bc(w_pose, (6,))),
                                                     int(frame), _p(bc(period, (B, 3))), C.c_double(w_increasing.max_weight), C.c_double(rate)))

    # -- streamed resident trajectory -----------------------------------------
    def stream_trajectory(self, capacity, max_span, w_q, w_qdot, w_effort, w_pose, frame):
        """An empty ring of `capacity` samples per instance for windows of up to `max_span` samples (agx_traj_stream_create):
        stream_append adds samples, stream_release drops the past, and set_window / mpc_step / traj_point / traj_tile take
        LOGICAL sample indexes (0 = the first sample ever appended)."""
        nv = self.nv
        bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        _chk(lib().agx_traj_stream_create(self._h, int(capacity), int(max_span), _p(bc(w_q, (nv,))), _p(bc(w_qdot, (nv,))),
                                          _p(bc(w_effort, (nv,))), _p(bc(w_pose, (6,))), int(frame)))

    def stream_append(self, q, dq, ddq, pose=None, w_pose=None, w_collision=None):
        """Appends m samples per instance: q, dq, ddq [B][m][nv]; pose [B][m][12], w_pose [B][m][6], w_collision [B][m] optional (they
        broadcast over B), as in generic_trajectory_weighted.  The arrays may be reused at once; the device work runs on the
        handle's copy stream beside the solver (agx_traj_stream_append states the ordering)."""
        B, nv = self.B, self.nv
        q = _f8(q)
        if q.ndim != 3 or q.shape[0] != B or q.shape[2] != nv:
            raise ValueError(f"q: expected shape ({B}, m, {nv}), got {q.shape}")
        m = q.shape[1]
        dq, ddq = _f8(dq, (B, m, nv)), _f8(ddq, (B, m, nv))
        bc = lambda a, shape: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))  # noqa: E731
        _chk(lib().agx_traj_stream_append(self._h, int(m), _p(q), _p(dq), _p(ddq), _p(bc(pose, (B, m, 12))), _p(bc(w_pose, (B, m, 6))),
                                          _p(bc(w_collision, (B, m)))))

    def stream_release(self, k: int):
        """Samples below logical index k are no longer needed (TrajectoryBuffer.clear_past, several at once if wanted)."""
        _chk(lib().agx_traj_stream_release(self._h, int(k)))

    def stream_range(self):
        """(first, end): the retained logical samples are [first, end)."""
        first, end = C.c_int(0), C.c_int(0)
        _chk(lib().agx_traj_stream_range(self._h, C.byref(first), C.byref(end)))
        return first.value, end.value

    def stream_joins(self):
        """(joins, pending): how often the solver stream was made to wait for an append, and the appended pieces not joined yet
        (debug reader of the ordering contract of agx_traj_stream_append)."""
        joins, pending = C.c_longlong(0), C.c_int(0)
        _chk(lib().agx_traj_stream_joins(self._h, C.byref(joins), C.byref(pending)))
        return joins.value, pending.value

    def stream_timing(self, enable: bool):
        """Switch the in-situ timing of the two streams on/off; returns (ms_sum[2], count[2]) accumulated so far:
        [0] the solver stream waiting for fills, [1] transfer + fill of the appended pieces on the copy stream."""
        ms = (C.c_double * 2)()
        cnt = (C.c_longlong * 2)()
        _chk(lib().agx_traj_stream_timing(self._h, 1 if enable else 0, ms, cnt))
        return list(ms), list(cnt)

    def set_horizon_indexes(self, idx):
        """TrajectoryBuffer.horizon_indexes for the resident trajectory (None = uniform)."""
        a = None if idx is None else np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(self.T + 1))
        _chk(lib().agx_traj_set_horizon_indexes(self._h, _p(a)))

    def set_window(self, k0: int):
        _chk(lib().agx_traj_set_window(self._h, int(k0)))

    def traj_point(self, k: int):
        B, nv = self.B, self.nv
        q, v, a, u = (np.empty((B, nv)) for _ in range(4))
        pose = np.empty((B, 12))
        _chk(lib().agx_traj_get_point(self._h, int(k), _p(q), _p(v), _p(a), _p(u), _p(pose)))
        return q, v, a, u, pose

    def traj_tile(self, k: int, terminal: bool = False):
        """Reference tile [B][stride] of resident sample k in the running or the terminal layout (`PackedOcp.row_view` offsets).
        A debug reader: it ends the tile carry."""
        out = np.empty((self.B, self.stride))
        _chk(lib().agx_traj_get_tile(self._h, int(k), 1 if terminal else 0, _p(out)))
        return out

    def warmstart_from_reference(self):
        _chk(lib().agx_traj_warmstart_from_reference(self._h))

    def mpc_step(self, k0: int, max_iter: int, first):
        """first: True/1 warm start from the reference, False/0 x0 <- previous xs[1], 2 x0 as set by the caller."""
        _chk(lib().agx_ocp_mpc_step(self._h, int(k0), int(max_iter), int(first)))

    def download_x0(self):
        x0 = np.empty((self.B, self.nx))
        _chk(lib().agx_ocp_download_x0(self._h, _p(x0)))
        return x0

    def feedback_rollout(self, n_substeps: int, dt_sub: float, disturbance=None):
        """u = us[0] + K[0] (x0 - x) on the model for n_substeps of dt_sub; the end state becomes x0."""
        d = None if disturbance is None else _f8(disturbance).reshape(self.B, self.nu)
        _chk(lib().agx_ocp_feedback_rollout(self._h, int(n_substeps), C.c_double(dt_sub), _p(d)))

    # -- plant of the closed loop ---------------------------------------------
    def _plant_arg(self, name, a, tail):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        want = (self.B, self.nv) + tail
        if tail == (9,) and a.shape == (self.B, self.nv, 3, 3):
            a = a.reshape(want)
        if a.shape != want:
            raise ValueError(f"{name}: expected shape {want}, got {a.shape}")
        return a

    def set_plant_inertials(self, mass, com, inertia, armature=None):
        """Per-instance link inertials of the robot feedback_rollout simulates (`workloads.stack_inertials` of B tables):
        mass [B][nv], com [B][nv][3], inertia [B][nv][9] (or [B][nv][3][3]), armature [B][nv] (None: the model's).  The
        controller keeps its own model."""
        mass, com, inertia = self._plant_arg("mass", mass, ()), self._plant_arg("com", com, (3,)), self._plant_arg("inertia", inertia, (9,))
        arm = None if armature is None else self._plant_arg("armature", armature, ())
        _chk(lib().agx_ocp_set_plant_inertials(self._h, _p(mass), _p(com), _p(inertia), _p(arm)))

    def clear_plant_inertials(self):
        """feedback_rollout simulates the controller's own model again."""
        _chk(lib().agx_ocp_set_plant_inertials(self._h, None, None, None, None))

    # -- controller model per instance -------------------------------------------
    def set_model_inertials(self, mass, com, inertia, armature=None):
        """Per-instance link inertials of the model instance b SOLVES with (`workloads.stack_inertials` of B tables), arrays as
        `set_plant_inertials`.  Derivative passes, the warm-start shift and -- with no plant set -- feedback_rollout read them;
        integrate, rnea, the frame functions, model_sensitivity and the trajectory generators keep the model's own table.
        Models of at most 7 joints after padding, no ControlGrav item."""
        mass, com, inertia = self._plant_arg("mass", mass, ()), self._plant_arg("com", com, (3,)), self._plant_arg("inertia", inertia, (9,))
        arm = None if armature is None else self._plant_arg("armature", armature, ())
        _chk(lib().agx_ocp_set_model_inertials(self._h, _p(mass), _p(com), _p(inertia), _p(arm)))

    def clear_model_inertials(self):
        """Every instance solves with the model's own table again."""
        _chk(lib().agx_ocp_set_model_inertials(self._h, None, None, None, None))

    # -- obstacles per instance ----------------------------------------------------
    def set_obstacle_placements(self, frames, se3):
        """Per-instance placements of world-fixed geometry frames (`workloads.obstacle_placements`): `frames` n ids or names of
        the table, `se3` [B][n][12] (rotation row-major 9, then translation 3).  Instance b evaluates every collision cost and
        constraint row that names a listed frame at se3[b][slot]; frames that are not listed keep the model's placement, a
        listed one ignores set_geom_placement until clear_obstacle_placements.  agx_model_frame_placement / _jacobian and the
        trajectory generators keep the model's table.  Models of at most 7 joints after padding."""
        ids = [self.table.frame_names.index(f) if isinstance(f, str) else int(f) for f in np.asarray(frames, dtype=object).reshape(-1)]
        n = len(ids)
        if n < 1:
            raise ValueError("frames: expected at least one frame (clear_obstacle_placements drops the table)")
        a = np.asarray(se3)
        if a.shape == (self.B, n, 3, 4) or a.shape == (self.B, n, 4, 4):
            raise ValueError(f"se3: expected shape {(self.B, n, 12)} (rotation row-major 9, then translation 3), got the matrix form {a.shape}")
        if a.shape != (self.B, n, 12):
            raise ValueError(f"se3: expected shape {(self.B, n, 12)}, got {a.shape}")
        a = np.ascontiguousarray(a, dtype=np.float64)
        fr = np.ascontiguousarray(ids, dtype=np.int32)
        _chk(lib().agx_ocp_set_obstacle_placements(self._h, C.c_int(n), _p(fr), _p(a)))

    def clear_obstacle_placements(self):
        """Every instance sees the model's own placements again (the latest set_geom_placement included)."""
        _chk(lib().agx_ocp_set_obstacle_placements(self._h, C.c_int(0), None, None))

    def model_sensitivity(self, x, u, dt, delta_inertia=0.01, delta_com=0.01, delta_mass=0.01):
        """[n][2 nv][10 nv] sensitivity of the Euler node's next state to the link inertials of the controller's model at the
        samples x [n][nx], u [n][nu] (agx_model_sensitivity; `workloads.sensitivity_columns` labels the columns)."""
        x, u = np.ascontiguousarray(np.asarray(x, dtype=np.float64)), np.ascontiguousarray(np.asarray(u, dtype=np.float64))
        if x.ndim != 2 or x.shape[1] != self.nx or x.shape[0] < 1:
            raise ValueError(f"x: expected shape (n, {self.nx}), got {x.shape}")
        if u.shape != (x.shape[0], self.nu):
            raise ValueError(f"u: expected shape ({x.shape[0]}, {self.nu}), got {u.shape}")
        out = np.empty((x.shape[0], 2 * self.nv, 10 * self.nv))
        _chk(lib().agx_model_sensitivity(self._h, int(x.shape[0]), C.c_double(dt), _p(x), _p(u), C.c_double(delta_inertia),
                                         C.c_double(delta_com), C.c_double(delta_mass), _p(out)))
        return out
