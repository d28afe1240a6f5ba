"""Python front-end of the explicit-scalar entry points (``include/c21cm_grid.h``).

Inputs may be numpy arrays (host memory -- the library stages them, which is the
py21cmfast/CFFI situation) or torch CUDA tensors (HBM -- used in place).  Outputs are
created in the same kind of memory as ``density``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import structs as S
from ._lib import check, load


def _is_torch(a) -> bool:
    return a is not None and type(a).__module__.startswith("torch")


def _fptr(a):
    if a is None:
        return None
    if _is_torch(a):
        assert a.is_contiguous() and a.dtype.is_floating_point and a.element_size() == 4
        return C.cast(a.data_ptr(), S.c_float_p)
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(S.c_float_p)


def _vptr(a):
    if a is None:
        return None
    if _is_torch(a):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _new_like(ref, fill: float, dtype=None):
    if _is_torch(ref):
        import torch

        return torch.full(ref.shape, fill, dtype=dtype or torch.float32, device=ref.device)
    return np.full(ref.shape, fill, dtype or np.float32)


def _stack_like(ref, n: int):
    """zeros of shape (n, *ref.shape), float32, where ``ref`` lives"""
    if _is_torch(ref):
        import torch

        return torch.zeros((n,) + tuple(ref.shape), dtype=torch.float32, device=ref.device)
    return np.zeros((n,) + tuple(ref.shape), np.float32)


def _stream(stream):
    if stream is not None:
        return C.c_void_p(stream)
    try:
        import torch

        if torch.cuda.is_available():
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    except Exception:
        pass
    return C.c_void_p(0)


def fft_r2c(padded, nx, ny, nz, stream=None):
    check(load().c21cm_fft_r2c(_vptr(padded), nx, ny, nz, _stream(stream)), "c21cm_fft_r2c")


def fft_c2r(padded, nx, ny, nz, stream=None):
    check(load().c21cm_fft_c2r(_vptr(padded), nx, ny, nz, _stream(stream)), "c21cm_fft_c2r")


def filter_grid(box, box_len, filter_type, R, R_param=0.0, box_len_z=None, stream=None):
    """r2c -> /N -> W(kR) -> c2r of one box (reference: filtering.c:397-445)."""
    nx, ny, nz = box.shape
    out = _new_like(box, 0.0)
    check(
        load().c21cm_filter_grid(_vptr(box), _vptr(out), nx, ny, nz, box_len,
                                 box_len if box_len_z is None else box_len_z, filter_type, R,
                                 R_param, _stream(stream)),
        "c21cm_filter_grid",
    )
    return out


class IonizeBuffers:
    """Owns the output arrays of one IonizedBox (what ``IonizedBox.new`` allocates in
    py21cmfast, reference: src/py21cmfast/wrapper/outputs.py:1475-1545)."""

    def __init__(self, density, need_nion: bool = False, minimize_memory: bool = False,
                 recomb_model: int = 0, mini_radii: int = 0):
        self.neutral_fraction = _new_like(density, 1.0)  # initialised to ones (:1524-1527)
        self.z_reion = _new_like(density, 0.0)
        self.kinetic_temperature = None if minimize_memory else _new_like(density, 0.0)
        self.unnormalised_nion = _new_like(density, 0.0) if need_nion else None
        self.unnormalised_nion_mini = None
        if mini_radii:  # USE_MINI_HALOS: one f_coll grid per filter radius (:1538-1543)
            stack = _stack_like(density, mini_radii)
            self.unnormalised_nion = stack
            self.unnormalised_nion_mini = _stack_like(density, mini_radii)
        # recombination models (:1526-1537): Gamma_12 and the mean free path are always part of
        # the reference's IonizedBox; here they are only allocated when something writes them
        self.ionisation_rate_G12 = self.mean_free_path = self.cumulative_recombinations = None
        if recomb_model:
            self.ionisation_rate_G12 = _new_like(density, 0.0)
            if not minimize_memory:
                self.mean_free_path = _new_like(density, 0.0)
            if recomb_model == 2:
                self.cumulative_recombinations = _new_like(density, 0.0)
            else:  # homogeneous: one number, shape (1, 1, 1)
                self.cumulative_recombinations = _new_like(density[:1, :1, :1], 0.0)

    def reset(self):
        """Back to the state of a freshly allocated IonizedBox.  z_reion needs no reset: every
        ComputeIonizedBox path overwrites it (IonisationBox.c:1372-1378 fills it with -1)."""
        self.neutral_fraction[...] = 1.0
        if self.kinetic_temperature is not None:
            self.kinetic_temperature[...] = 0.0
        for a in (self.ionisation_rate_G12, self.mean_free_path, self.cumulative_recombinations):
            if a is not None:
                a[...] = 0.0

    def struct(self) -> S.IonizedBoxStruct:
        return S.IonizedBoxStruct(
            neutral_fraction=_fptr(self.neutral_fraction), z_reion=_fptr(self.z_reion),
            kinetic_temperature=_fptr(self.kinetic_temperature),
            unnormalised_nion=_fptr(self.unnormalised_nion),
            unnormalised_nion_mini=_fptr(self.unnormalised_nion_mini),
            ionisation_rate_G12=_fptr(self.ionisation_rate_G12),
            mean_free_path=_fptr(self.mean_free_path),
            cumulative_recombinations=_fptr(self.cumulative_recombinations),
        )


def _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec=None, whalo_sfr=None):
    pf = S.PerturbedFieldStruct(density=_fptr(density))
    prev = S.IonizedBoxStruct(z_reion=_fptr(prev_z_reion),
                              cumulative_recombinations=_fptr(prev_nrec))
    ts = S.TsBoxStruct(xray_ionised_fraction=_fptr(xe), kinetic_temp_neutral=_fptr(Tneutral))
    hb = S.HaloBoxStruct(n_ion=_fptr(n_ion), whalo_sfr=_fptr(whalo_sfr))
    return pf, prev, ts, hb


def ionize_grids(spec: S.IonizeSpec, density, n_ion=None, xe=None, Tneutral=None,
                 prev_z_reion=None, buffers: IonizeBuffers | None = None, stream=None,
                 prev_nrec=None, whalo_sfr=None, mini=None):
    """One ComputeIonizedBox grid pass on the MI355X.  Returns (buffers, box_struct, report).
    ``prev_nrec`` (the previous box's cumulative_recombinations) and ``whalo_sfr`` (HaloBox) are
    the extra inputs of the recombination models.  ``mini`` (USE_MINI_HALOS): dict with
    prev_density, log10_mturn_acg, log10_mturn_mcg [N] and prev_nion, prev_nion_mini
    [n_radii, N] (the previous box's per-radius f_coll history), numpy or CUDA tensors."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory),
                                recomb_model=spec.recomb_model,
                                mini_radii=spec.n_radii if mini is not None else 0)
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec,
                                      whalo_sfr)
    if mini is not None:
        spec.prev_density = _fptr(mini["prev_density"])
        spec.log10_mturn_acg = _fptr(mini["log10_mturn_acg"])
        spec.log10_mturn_mcg = _fptr(mini["log10_mturn_mcg"])
        prev.unnormalised_nion = _fptr(mini["prev_nion"])
        prev.unnormalised_nion_mini = _fptr(mini["prev_nion_mini"])
    box = buffers.struct()
    rep = S.IonizeReport()
    check(
        load().c21cm_ionize_grids(C.byref(spec), C.byref(pf), C.byref(prev), C.byref(ts),
                                  C.byref(hb), C.byref(box), C.byref(rep), _stream(stream)),
        "c21cm_ionize_grids",
    )
    return buffers, box, rep


def mturn_grids(spec: S.MturnSpec, prev_G12, prev_z_reion, J_21_LW, vcb=None, stream=None):
    """calculate_mcrit_boxes on the device: (log10 M_turn,a, log10 M_turn,m, <a>, <m>); the
    grids are allocated like ``J_21_LW`` (numpy array or CUDA tensor)."""
    a, m = _new_like(J_21_LW, 0.0), _new_like(J_21_LW, 0.0)
    ave_a, ave_m = C.c_double(), C.c_double()
    check(
        load().c21cm_mturn_grids(C.byref(spec), _vptr(prev_G12), _vptr(prev_z_reion),
                                 _vptr(J_21_LW), _vptr(vcb), _vptr(a), _vptr(m), C.byref(ave_a),
                                 C.byref(ave_m), _stream(stream)),
        "c21cm_mturn_grids",
    )
    return a, m, ave_a.value, ave_m.value


def ionize_shard_radii(spec, rank, world, first_cross, density, n_ion=None, xe=None,
                       Tneutral=None, prev_z_reion=None, stream=None, want_report=True):
    """Shard phase: this rank's radii -> ``first_cross`` (uint8 CUDA tensor).
    ``want_report=False`` skips the per-radius f_coll means and with them the host
    synchronisation at the end of the phase (the call only enqueues work)."""
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion)
    rep = S.IonizeReport() if want_report else None
    check(
        load().c21cm_ionize_shard_radii(C.byref(spec), rank, world, C.byref(pf), C.byref(prev),
                                        C.byref(ts), C.byref(hb),
                                        C.c_void_p(first_cross.data_ptr()),
                                        C.byref(rep) if want_report else None,
                                        _stream(stream)),
        "c21cm_ionize_shard_radii",
    )
    return rep


def ionize_shard_set_means(means):
    """Hand the rank-summed per-radius f_coll grid means to the next finish step."""
    m = np.ascontiguousarray(means, np.float64)
    lib = load()
    lib.c21cm_ionize_shard_set_means.restype = C.c_int
    lib.c21cm_ionize_shard_set_means.argtypes = [C.c_void_p, C.c_int]
    check(lib.c21cm_ionize_shard_set_means(m.ctypes.data_as(C.c_void_p), int(m.size)),
          "c21cm_ionize_shard_set_means")


def ionize_shard_finish(spec, first_cross, density, n_ion=None, xe=None, Tneutral=None,
                        prev_z_reion=None, buffers: IonizeBuffers | None = None, stream=None):
    """Finish phase on the owning rank: apply the reduced mask, radius 0, post-loop."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory))
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion)
    box = buffers.struct()
    rep = S.IonizeReport()
    check(
        load().c21cm_ionize_shard_finish(C.byref(spec), C.c_void_p(first_cross.data_ptr()),
                                         C.byref(pf), C.byref(prev), C.byref(ts), C.byref(hb),
                                         C.byref(box), C.byref(rep), _stream(stream)),
        "c21cm_ionize_shard_finish",
    )
    return buffers, box, rep


class ShardSlabState(C.Structure):
    """c21cm_shard_slab_state (include/c21cm_grid.h): what the exchange callback of the slab finish sees."""
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("n_chunks", C.c_int), ("chunk_begin", C.c_int),
                ("chunk_end", C.c_int), ("chunk_cells", C.c_size_t), ("cell_begin", C.c_size_t),
                ("cell_end", C.c_size_t), ("ntot", C.c_size_t), ("partials_stars", C.c_void_p),
                ("partials_xh", C.c_void_p), ("flag", C.c_void_p), ("out", C.c_void_p * 3)]


SLAB_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(ShardSlabState), C.c_int, C.c_void_p)


def shard_slab_supported(spec) -> bool:
    """Does the finish phase of this model run by cell slabs (c21cm_ionize_shard_slab_supported)?"""
    lib = load()
    lib.c21cm_ionize_shard_slab_supported.restype = C.c_int
    return bool(lib.c21cm_ionize_shard_slab_supported(C.byref(spec)))


def shard_slab(spec, rank: int, world: int) -> dict:
    """Chunks and cells of `rank`'s slab of the final sweep (c21cm_ionize_shard_slab)."""
    lib = load()
    lib.c21cm_ionize_shard_slab.restype = C.c_int
    cb, ce, nch = C.c_int(), C.c_int(), C.c_int()
    c0, c1, cc = C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(lib.c21cm_ionize_shard_slab(C.byref(spec), C.c_int(rank), C.c_int(world), C.byref(cb),
                                      C.byref(ce), C.byref(c0), C.byref(c1), C.byref(nch), C.byref(cc)),
          "c21cm_ionize_shard_slab")
    return {"chunk_begin": cb.value, "chunk_end": ce.value, "cell_begin": c0.value,
            "cell_end": c1.value, "n_chunks": nch.value, "chunk_cells": cc.value}


class _DevView:
    """A raw device address as a CUDA array (torch.as_tensor reads __cuda_array_interface__)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False),
                                         "version": 2}


def device_view(ptr: int, n: int, kind: str):
    """torch view (no copy) of n elements at a device address; kind: 'f8', 'f4', 'i4'."""
    import torch

    return torch.as_tensor(_DevView(ptr, n, "<" + kind), device="cuda")


def ionize_shard_finish_slab(spec, first_cross, rank, world, density, n_ion=None, xe=None,
                             Tneutral=None, prev_z_reion=None, buffers: IonizeBuffers | None = None,
                             exchange=None, outputs_gathered=False, stream=None):
    """Finish phase of `rank` by cell slabs (c21cm_ionize_shard_finish_slab): the final sweep over the
    rank's chunks from the combined first crossings of that slab, `exchange(state, local_status)`
    (a Python callable: all-gathers the chunk sums -- and the output slabs if the caller wants whole
    boxes -- and returns the agreed status), then the fixed-order reduce and the post-loop on every
    rank.  Returns (buffers, box_struct, report); the outputs are valid on the rank's slab
    (everywhere with ``outputs_gathered``)."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory))
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion)
    box = buffers.struct()
    rep = S.IonizeReport()
    lib = load()
    lib.c21cm_ionize_shard_finish_slab.restype = C.c_int
    err = []

    def _cb(user, state, local_status, strm):
        try:
            return int(exchange(state.contents, local_status) or 0)
        except Exception as e:  # an exception must not unwind through the C frames
            err.append(e)
            return 3

    cb = SLAB_EXCHANGE_FN(_cb) if exchange is not None else C.cast(None, SLAB_EXCHANGE_FN)
    st = lib.c21cm_ionize_shard_finish_slab(
        C.byref(spec), C.c_void_p(first_cross.data_ptr()), C.c_int(rank), C.c_int(world), C.byref(pf),
        C.byref(prev), C.byref(ts), C.byref(hb), C.byref(box), C.byref(rep), cb, None,
        C.c_int(1 if outputs_gathered else 0), _stream(stream))
    if err:
        raise err[0]
    check(st, "c21cm_ionize_shard_finish_slab")
    return buffers, box, rep


def shard_pack_mask_bits(first_cross, stream=None):
    """uint8 first crossings -> one bit per cell (uint32 words; c21cm_shard_pack_mask_bits)."""
    import torch

    n = first_cross.numel()
    bits = torch.empty((n + 31) // 32, dtype=torch.int32, device=first_cross.device)
    lib = load()
    lib.c21cm_shard_pack_mask_bits.restype = C.c_int
    check(lib.c21cm_shard_pack_mask_bits(C.c_void_p(first_cross.data_ptr()), C.c_void_p(bits.data_ptr()),
                                         C.c_size_t(n), _stream(stream)), "c21cm_shard_pack_mask_bits")
    return bits


def shard_or_unpack_mask_bits(pieces, first_cross_slab, stream=None):
    """OR of the packed pieces (2-D int32 [world][words]) into the uint8 cells of a slab
    (c21cm_shard_or_unpack_mask_bits)."""
    lib = load()
    lib.c21cm_shard_or_unpack_mask_bits.restype = C.c_int
    world, words = pieces.shape
    check(lib.c21cm_shard_or_unpack_mask_bits(C.c_void_p(pieces.data_ptr()), C.c_size_t(words),
                                              C.c_int(world), C.c_void_p(first_cross_slab.data_ptr()),
                                              C.c_size_t(first_cross_slab.numel()), _stream(stream)),
          "c21cm_shard_or_unpack_mask_bits")
    return first_cross_slab


def ionize_shard_radii_keys(spec, rank, world, cross_keys, density, n_ion=None, xe=None,
                            Tneutral=None, prev_z_reion=None, prev_nrec=None, whalo_sfr=None,
                            stream=None):
    """Shard phase of a recombination model: this rank's radii -> ``cross_keys`` (int64 / uint64
    CUDA tensor of N entries: bits(mean free path) << 32 | bits(Gamma_12), 0 = not crossed)."""
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec,
                                      whalo_sfr)
    lib = load()
    lib.c21cm_ionize_shard_radii_keys.restype = C.c_int
    check(lib.c21cm_ionize_shard_radii_keys(C.byref(spec), C.c_int(rank), C.c_int(world),
                                            C.byref(pf), C.byref(prev), C.byref(ts), C.byref(hb),
                                            C.c_void_p(cross_keys.data_ptr()), None,
                                            _stream(stream)),
          "c21cm_ionize_shard_radii_keys")


def ionize_shard_finish_keys(spec, cross_keys, density, n_ion=None, xe=None, Tneutral=None,
                             prev_z_reion=None, prev_nrec=None, whalo_sfr=None,
                             buffers: IonizeBuffers | None = None, stream=None):
    """Finish phase of a recombination model on the owning rank (reduced keys in)."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory),
                                recomb_model=spec.recomb_model)
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec,
                                      whalo_sfr)
    box = buffers.struct()
    rep = S.IonizeReport()
    lib = load()
    lib.c21cm_ionize_shard_finish_keys.restype = C.c_int
    check(lib.c21cm_ionize_shard_finish_keys(C.byref(spec), C.c_void_p(cross_keys.data_ptr()),
                                             C.byref(pf), C.byref(prev), C.byref(ts), C.byref(hb),
                                             C.byref(box), C.byref(rep), _stream(stream)),
          "c21cm_ionize_shard_finish_keys")
    return buffers, box, rep


def ionize_last_loop_flags() -> int:
    """Which R loop the last ionisation call set up (c21cm_ionize_last_loop_flags): 1 fused, 2 fused
    recombination loop, 4 third spectrum in the barrier kernel, 8 ... which is the filtered N_rec, 16 a
    fourth spectrum (x_e and filtered N_rec), 32 two radii per sweep, 64 the Eulerian loops' cell-scale radius and
    post-loop ran as one sweep (set by the finish of that call)."""
    lib = load()
    lib.c21cm_ionize_last_loop_flags.restype = C.c_int
    return int(lib.c21cm_ionize_last_loop_flags())


def shard_rc_supported(spec) -> bool:
    """Does a recombination spec shard through the fused loop (first-crossing index + Gamma_12,
    5 bytes per cell) rather than through the 64-bit keys?  c21cm_ionize_shard_rc_supported."""
    return bool(load().c21cm_ionize_shard_rc_supported(C.byref(spec)))


def ionize_shard_radii_rc(spec, rank, world, first_cross, cross_g12, density, n_ion=None,
                          prev_z_reion=None, prev_nrec=None, whalo_sfr=None, xe=None, Tneutral=None,
                          stream=None):
    """Shard phase of the fused recombination loop: this rank's radii -> ``first_cross`` (uint8
    CUDA tensor, radius index of the first crossing, 0 = none) and ``cross_g12`` (float32,
    Gamma_12 at that crossing).  ``xe`` / ``Tneutral``: the TsBox grids of a spin-temperature run."""
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec, whalo_sfr)
    lib = load()
    lib.c21cm_ionize_shard_radii_rc.restype = C.c_int
    check(lib.c21cm_ionize_shard_radii_rc(C.byref(spec), C.c_int(rank), C.c_int(world), C.byref(pf),
                                          C.byref(prev), C.byref(ts), C.byref(hb),
                                          C.c_void_p(first_cross.data_ptr()),
                                          C.c_void_p(cross_g12.data_ptr()), None, _stream(stream)),
          "c21cm_ionize_shard_radii_rc")


def ionize_shard_finish_rc(spec, first_cross, cross_g12, density, n_ion=None, prev_z_reion=None,
                           prev_nrec=None, whalo_sfr=None, buffers: IonizeBuffers | None = None,
                           xe=None, Tneutral=None, stream=None):
    """Finish phase of the fused recombination loop on the owning rank (combined grids in)."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory),
                                recomb_model=spec.recomb_model)
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec, whalo_sfr)
    box = buffers.struct()
    rep = S.IonizeReport()
    lib = load()
    lib.c21cm_ionize_shard_finish_rc.restype = C.c_int
    check(lib.c21cm_ionize_shard_finish_rc(C.byref(spec), C.c_void_p(first_cross.data_ptr()),
                                           C.c_void_p(cross_g12.data_ptr()), C.byref(pf),
                                           C.byref(prev), C.byref(ts), C.byref(hb), C.byref(box),
                                           C.byref(rep), _stream(stream)),
          "c21cm_ionize_shard_finish_rc")
    return buffers, box, rep


def combine_cross_g12(mask, g12, peer_mask, peer_g12, stream=None):
    """c21cm_shard_combine_cross_g12: own slab (uint8 / float32 CUDA tensors, in place) against
    the peers' slabs ``peer_mask`` [n_peers, stride] / ``peer_g12`` [n_peers, stride]."""
    lib = load()
    lib.c21cm_shard_combine_cross_g12.restype = C.c_int
    n_peers, stride = peer_mask.shape
    check(lib.c21cm_shard_combine_cross_g12(C.c_void_p(mask.data_ptr()), C.c_void_p(g12.data_ptr()),
                                            C.c_void_p(peer_mask.data_ptr()),
                                            C.c_void_p(peer_g12.data_ptr()), C.c_int(n_peers),
                                            C.c_size_t(stride), C.c_size_t(mask.numel()),
                                            _stream(stream)),
          "c21cm_shard_combine_cross_g12")


PLACEMENT_OUTCOMES = ("placed against the partner by timed launches", "off / not applicable",
                      "other tenants on the device", "another process was walking", "no faster candidate in the budget",
                      "an earlier walk for this size found nothing", "tenancy unknown and the device is busy",
                      "the walk's time budget ran out")


def placement_report():
    """What the last placement decision of a work spectrum was and what it cost (csrc/host/placement.c:
    c21cm_placement_report); None before any."""
    lib = load()
    out = (C.c_double * 8)()
    lib.c21cm_placement_report.restype = C.c_int
    if lib.c21cm_placement_report(out) != 0:
        return None
    return {"outcome": PLACEMENT_OUTCOMES[int(out[0])], "held_GB": round(out[1], 2), "probes": int(out[2]),
            "chosen_ms": round(out[3], 4), "first_candidate_ms": round(out[4], 4), "decision_wall_ms": round(out[5], 2),
            "tenants": int(out[6]), "walks": int(out[7])}


def placement_set(mode: int):
    """Opt into (1; 2 = also on a shared device) or out of (0) the placement walk of the work spectra; -1: the
    environment's C21CM_WS_PLACE (unset: off).  csrc/host/placement.c."""
    lib = load()
    lib.c21cm_placement_set.restype = C.c_int
    check(lib.c21cm_placement_set(C.c_int(mode)), "c21cm_placement_set")


def shard_init_from_torch(group=None):
    """Bootstrap the library's own RCCL communicator from an initialised ``torch.distributed``
    job: rank 0 draws the unique id in C (c21cm_shard_unique_id), torch broadcasts its 128 bytes,
    every rank calls c21cm_shard_init.  Afterwards the exchange of the sharded R loop happens
    inside the C library (c21cm_ionize_sharded, and ComputeIonizedBox itself)."""
    import torch
    import torch.distributed as dist

    lib = load(require_gpu=True)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    buf = (C.c_ubyte * 128)()
    if rank == 0:
        check(lib.c21cm_shard_unique_id(buf), "c21cm_shard_unique_id")
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.tensor(list(buf), dtype=torch.uint8, device=dev)
    dist.broadcast(t, src=0, group=group)
    raw = bytes(t.cpu().tolist())
    check(lib.c21cm_shard_init(C.c_int(rank), C.c_int(world), raw), "c21cm_shard_init")
    return rank, world


def shard_init_single():
    """A one-rank communicator (plumbing tests on a single GPU)."""
    lib = load(require_gpu=True)
    buf = (C.c_ubyte * 128)()
    check(lib.c21cm_shard_unique_id(buf), "c21cm_shard_unique_id")
    check(lib.c21cm_shard_init(0, 1, bytes(buf)), "c21cm_shard_init")


def shard_emulate(rank: int, world: int, mailbox):
    """Test hook (c21cm_shard_emulate): run the ranks of a world > 1 job one after the other in
    this process against the device ``mailbox`` (uint8 CUDA tensor, zeroed per round)."""
    lib = load(require_gpu=True)
    lib.c21cm_shard_emulate.restype = C.c_int
    check(lib.c21cm_shard_emulate(C.c_int(rank), C.c_int(world), C.c_void_p(mailbox.data_ptr()),
                                  C.c_size_t(mailbox.numel())), "c21cm_shard_emulate")


def shard_finalize():
    load().c21cm_shard_finalize()


def ionize_sharded(spec: S.IonizeSpec, density, n_ion=None, xe=None, Tneutral=None,
                   prev_z_reion=None, buffers: IonizeBuffers | None = None, stream=None,
                   prev_nrec=None, whalo_sfr=None, broadcast=False):
    """One ComputeIonizedBox pass with the R loop sharded over the ranks of the library's RCCL
    communicator (c21cm_ionize_sharded), all inside the C library: shard phase, exchange, finish.
    Where the finish phase runs by cell slabs (``shard_slab_supported``) every rank finishes its slab
    and holds the complete scalars; otherwise the owner rank finishes.  Returns (buffers, box_struct,
    report); ``broadcast``: True / 1 whole boxes on every rank, 2 the whole neutral-fraction box on every
    rank (slab finish, device arrays), False / 0 a rank's slab / the owner's box, None the library's
    default (c21cm_shard_output_mode)."""
    if buffers is None:
        buffers = IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                minimize_memory=bool(spec.minimize_memory),
                                recomb_model=spec.recomb_model)
    pf, prev, ts, hb = _input_structs(density, n_ion, xe, Tneutral, prev_z_reion, prev_nrec,
                                      whalo_sfr)
    box = buffers.struct()
    rep = S.IonizeReport()
    lib = load()
    lib.c21cm_ionize_sharded.restype = C.c_int
    check(lib.c21cm_ionize_sharded(C.byref(spec), C.byref(pf), C.byref(prev), C.byref(ts),
                                   C.byref(hb), C.byref(box), C.byref(rep),
                                   C.c_int(-1 if broadcast is None else int(broadcast)),
                                   _stream(stream)),
          "c21cm_ionize_sharded")
    return buffers, box, rep


IC_FIELDS = ("lowres_density", "lowres_vx", "lowres_vy", "lowres_vz", "lowres_vx_2LPT",
             "lowres_vy_2LPT", "lowres_vz_2LPT", "hires_density", "hires_vx", "hires_vy",
             "hires_vz", "hires_vx_2LPT", "hires_vy_2LPT", "hires_vz_2LPT", "lowres_vcb")


def ics_struct(ics: dict) -> S.InitialConditionsStruct:
    """InitialConditions struct over a dict of numpy arrays / torch tensors (missing -> NULL)."""
    return S.InitialConditionsStruct(**{k: _fptr(ics.get(k)) for k in IC_FIELDS})


def perturb_grids(spec: S.PerturbSpec, ics: dict, stream=None) -> dict:
    """ComputePerturbedField grid algorithm on the MI355X.

    Outputs live where ``ics['hires_density']`` (or lowres_density for LINEAR) lives.
    Shapes as py21cmfast's PerturbedField.new (reference: wrapper/outputs.py:689-719).
    """
    ref = ics.get("hires_density")
    if ref is None:
        ref = ics["lowres_density"]
    lo = (spec.hii_dim, spec.hii_dim, spec.hii_dim_z)

    def new():
        if _is_torch(ref):
            import torch

            return torch.zeros(lo, dtype=torch.float32, device=ref.device)
        return np.zeros(lo, np.float32)

    out = {"density": new(), "velocity_z": new()}
    if spec.keep_3d_velocities:
        out["velocity_x"] = new()
        out["velocity_y"] = new()
    pf = S.PerturbedFieldStruct(**{k: _fptr(v) for k, v in out.items()})
    icss = ics_struct(ics)
    check(load().c21cm_perturb_grids(C.byref(spec), C.byref(icss), C.byref(pf), _stream(stream)),
          "c21cm_perturb_grids")
    return out


def new_ics_arrays(spec: S.IcsSpec, device=None) -> dict:
    """Zeroed arrays as ``InitialConditions.new`` allocates them
    (reference: src/py21cmfast/wrapper/outputs.py:534-581)."""
    lo = (spec.hii_dim, spec.hii_dim, spec.hii_dim_z)
    hi = (spec.dim, spec.dim, spec.dim_z)

    def new(shape):
        if device is not None:
            import torch

            return torch.zeros(shape, dtype=torch.float32, device=device)
        return np.zeros(shape, np.float32)

    ics = {"hires_density": new(hi), "lowres_density": new(lo)}
    shape = hi if spec.perturb_on_high_res else lo
    pre = "hires" if spec.perturb_on_high_res else "lowres"
    for ax in "xyz":
        ics[f"{pre}_v{ax}"] = new(shape)
        if spec.perturb_algorithm == 2:
            ics[f"{pre}_v{ax}_2LPT"] = new(shape)
    return ics


def ics_grids(spec: S.IcsSpec, ics: dict | None = None, device=None, stream=None) -> dict:
    """ComputeInitialConditions grid algorithm on the MI355X; fills and returns ``ics``."""
    if ics is None:
        ics = new_ics_arrays(spec, device)
    icss = ics_struct(ics)
    check(load().c21cm_ics_grids(C.byref(spec), C.byref(icss), _stream(stream)), "c21cm_ics_grids")
    return ics


def _int_array(a, itemsize: int, what: str):
    """A caller's integer array of `itemsize` bytes per element, host or device, as it is."""
    if _is_torch(a):
        assert a.is_contiguous() and not a.dtype.is_floating_point and a.element_size() == itemsize, what
    else:
        assert a.dtype.kind in "iu" and a.dtype.itemsize == itemsize and a.flags["C_CONTIGUOUS"], what
    return a


def gsl_raw_words(kind: int, seed: int, n: int, on_device: bool = False, out=None):
    """The first ``n`` raw outputs of generator ``kind`` (0 mt19937, 1 gfsr4, 2 cmrg, 3 mrg, 4 taus2) after
    ``gsl_rng_set(seed)``, computed on the host or on the device (the same words).  ``out``: a host or device
    array of 32-bit integers; default a new numpy uint32 array."""
    if out is None:
        out = np.zeros(n, np.uint32)
    _int_array(out, 4, "out")
    lib = load()
    lib.c21cm_gsl_raw_words.restype = C.c_int
    lib.c21cm_gsl_raw_words.argtypes = [C.c_int, C.c_ulonglong, C.c_size_t, C.c_int, C.c_void_p]
    check(lib.c21cm_gsl_raw_words(kind, seed, n, int(on_device), _vptr(out)), "c21cm_gsl_raw_words")
    return out


def gsl_accept_pairs(kind: int, words, want: int, on_device: bool = False):
    """The polar method's compaction on caller-supplied raw words of generator ``kind``: zero words dropped,
    survivors paired, pairs with 0 < x^2 + y^2 <= 1 kept as ``a | c << 32`` until ``want`` are found.
    ``words``: host or device array of 32-bit integers.  Returns (pairs as numpy uint64, words used)."""
    _int_array(words, 4, "words")
    n_words = words.numel() if _is_torch(words) else words.size
    pairs = np.zeros(max(1, min(want, n_words // 2)), np.uint64)
    n_pairs, n_used = C.c_size_t(), C.c_size_t()
    lib = load()
    lib.c21cm_gsl_accept_pairs.restype = C.c_int
    lib.c21cm_gsl_accept_pairs.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    check(lib.c21cm_gsl_accept_pairs(kind, _vptr(words), n_words, want, int(on_device), _vptr(pairs),
                                     C.byref(n_pairs), C.byref(n_used)), "c21cm_gsl_accept_pairs")
    return pairs[: n_pairs.value], n_used.value


def gsl_stream_pairs(seed: int, n_threads: int, shape, on_device: bool = False, max_pairs_per_launch: int = 0,
                     tile_cap: int = 0, out=None, stream=None):
    """The accepted raw pairs of the reference's IC draw -- ``seed_rng_threads(seed)`` with ``n_threads`` streams,
    two pairs per mode of a grid of ``shape`` = (nx, ny, nz) -- in grid order: (nx, ny, nz // 2 + 1, 2) packed
    ``a | c << 32``.  ``max_pairs_per_launch`` bounds one launch of the device draw (0: the default) and does not
    change the result; ``tile_cap`` bounds the tiles one launch may work through per stream (0: derived from the
    pairs asked for), and a launch that reaches it fails the call.  ``out``: a host or device array of 64-bit integers; default a new numpy uint64 array."""
    nx, ny, nz = shape
    nzc = nz // 2 + 1
    if out is None:
        out = np.zeros((nx, ny, nzc, 2), np.uint64)
    _int_array(out, 8, "out")
    assert (out.numel() if _is_torch(out) else out.size) == 2 * nx * ny * nzc
    lib = load()
    lib.c21cm_gsl_stream_pairs.restype = C.c_int
    lib.c21cm_gsl_stream_pairs.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_longlong, C.c_long, C.c_void_p, C.c_void_p]
    check(lib.c21cm_gsl_stream_pairs(seed, n_threads, nx, ny, nzc, int(on_device), max_pairs_per_launch, tile_cap,
                                     _vptr(out), _stream(stream) if on_device else None),
          "c21cm_gsl_stream_pairs")
    return out


def gsl_tile_words(kind: int = -1) -> int:
    """Words per tile of the device draw of generator ``kind``; -1: of ``gsl_accept_pairs``."""
    return int(load().c21cm_gsl_tile_words(kind))


def brightness_grids(spec: S.BrightnessSpec, density, neutral_fraction, spin_temperature=None,
                     stream=None) -> dict:
    """ComputeBrightnessTemp sweep on the MI355X (reference:
    src/py21cmfast/src/BrightnessTemperatureBox.c:22-105).  Outputs live where ``density`` lives.
    Returns dict(brightness_temp[, tau_21], mean)."""
    out = {"brightness_temp": _new_like(density, 0.0)}
    if spec.use_ts_fluct:
        out["tau_21"] = _new_like(density, 0.0)
    mean = C.c_double()
    check(load().c21cm_brightness_grids(C.byref(spec), _vptr(density), _vptr(neutral_fraction),
                                        _vptr(spin_temperature), _vptr(out["brightness_temp"]),
                                        _vptr(out.get("tau_21")), C.byref(mean), _stream(stream)),
          "c21cm_brightness_grids")
    out["mean"] = mean.value
    return out


def halobox_grids(spec: S.HaloBoxSpec, ics: dict, with_whalo=False, with_xray=False,
                  stream=None) -> dict:
    """ComputeHaloBox's grids on the MI355X (reference: src/py21cmfast/src/HaloBox.c:302-436,518-560,
    map_mass.c:214-476): the integrated branch and, when ``spec.halos`` / ``spec.halo_consts`` point at a
    catalogue (structs.halo_catalog, structs.HaloConsts), the halos deposited first
    (``spec.skip_integral``: halos only).  Outputs live where the source density lives.
    Returns dict(n_ion, halo_sfr[, whalo_sfr][, halo_xray][, halo_sfr_mini])."""
    ref = ics["hires_density" if spec.perturb_on_high_res else "lowres_density"]
    lo = (spec.hii_dim, spec.hii_dim, spec.hii_dim_z)

    def new():
        if _is_torch(ref):
            import torch

            return torch.zeros(lo, dtype=torch.float32, device=ref.device)
        return np.zeros(lo, np.float32)

    out = {"n_ion": new(), "halo_sfr": new()}
    if with_whalo:
        out["whalo_sfr"] = new()
    if with_xray:  # needs spec.ln_xray_table (USE_TS_FLUCT: the X-ray emissivity grid)
        out["halo_xray"] = new()
    if spec.use_mini_halos:  # the molecularly cooled star formation (HaloBox.c:271-277)
        out["halo_sfr_mini"] = new()
    hb = S.HaloBoxStruct(**{k: _fptr(v) for k, v in out.items()})
    icss = ics_struct(ics)
    check(load().c21cm_halobox_grids(C.byref(spec), C.byref(icss), C.byref(hb), _stream(stream)),
          "c21cm_halobox_grids")
    return out


def grid_minmax(values, stream=None):
    mm = (C.c_double * 2)()
    n = values.numel() if _is_torch(values) else values.size
    check(load().c21cm_grid_minmax(_vptr(values), C.c_size_t(n), mm, _stream(stream)),
          "c21cm_grid_minmax")
    return mm[0], mm[1]


def sampler_spec(redshift, redshift_desc=-1.0, seed=0) -> S.SampleHalosSpec:
    """The halo sampler's constants and tables of one snapshot from the broadcast globals
    (stoc_set_consts_z, Stochasticity.c:77-155): ``redshift_desc > 0`` for the progenitors of a catalogue at
    that redshift, else for the cells of the density grid.  ``spec.tables`` points at library-owned host
    tables that stay valid until the next call."""
    lib = load()
    lib.c21cm_sampler_setup.restype = C.c_int
    lib.c21cm_sampler_setup.argtypes = [C.c_double, C.c_double, C.c_ulonglong, C.c_void_p]
    spec = S.SampleHalosSpec()
    check(lib.c21cm_sampler_setup(float(redshift), float(redshift_desc), int(seed), C.byref(spec)),
          "c21cm_sampler_setup")
    return spec


def _catalog_of(cat):
    """HaloCatalogStruct of a struct, or of a dict of arrays (numpy or torch CUDA) with the reference's
    field names; None stays None"""
    if cat is None or isinstance(cat, S.HaloCatalogStruct):
        return cat
    n = int(cat["halo_masses"].shape[0])
    out = S.HaloCatalogStruct(n_halos=n, buffer_size=n)
    for name in ("halo_masses", "halo_coords", "star_rng", "sfr_rng", "xray_rng"):
        setattr(out, name, _fptr(cat[name]) if n else None)
    out._keep = cat
    return out


def sample_halos(spec: S.SampleHalosSpec, out: S.HaloCatalogStruct, density=None, overlap=None, large=None,
                 desc=None, stream=None):
    """The halo sampler on the MI355X (reference: Stochasticity.c:761-1113): the halos of every condition
    -- the descendant halos ``desc`` with ``spec.from_catalog``, else the cells of ``density`` [HII_DIM^3]
    (times D(z)), optionally after the ``large`` halos and with ``overlap`` taken off every cell -- appended
    to ``out`` (structs.empty_halo_catalog) in condition order, then draw order.  Arrays are numpy or torch
    CUDA tensors; catalogues are HaloCatalogStructs or dicts of such arrays.

    The random numbers are NOT the reference's GSL streams: every draw is a word of a Philox-4x32-10 block
    keyed by ``seed + int(1000 z)`` and counted by (condition, purpose, draw), another equally valid
    realisation that depends on nothing but the inputs.  Returns ``out`` (``n_halos`` set, arrays zero
    beyond it)."""
    lib = load()
    lib.c21cm_sample_halos_grids.restype = C.c_int
    lib.c21cm_sample_halos_grids.argtypes = [C.c_void_p, S.c_float_p, S.c_float_p] + [C.c_void_p] * 4
    large_s, desc_s = _catalog_of(large), _catalog_of(desc)
    check(lib.c21cm_sample_halos_grids(C.byref(spec), _fptr(density), _fptr(overlap),
                                       C.byref(large_s) if large_s is not None else None,
                                       C.byref(desc_s) if desc_s is not None else None, C.byref(out),
                                       _stream(stream)), "c21cm_sample_halos_grids")
    return out


def sample_halos_counts(n_conditions: int):
    """Halos kept per condition by the last ``sample_halos`` call (int32 numpy array): cuts its catalogue,
    which is in condition order, into the conditions."""
    lib = load()
    lib.c21cm_sample_halos_last_counts.restype = C.c_int
    lib.c21cm_sample_halos_last_counts.argtypes = [C.c_ulonglong, C.c_void_p]
    counts = np.zeros(int(n_conditions), np.int32)
    check(lib.c21cm_sample_halos_last_counts(int(n_conditions), counts.ctypes.data_as(C.c_void_p)),
          "c21cm_sample_halos_last_counts")
    return counts


def dexm_spec(redshift, seed=0) -> S.FindHalosSpec:
    """The DexM radius ladder of one snapshot from the broadcast globals (HaloCatalog.c:81-200): the kept
    rungs (R, M, delta_crit), the growth factor and the options.  ``n_R == 0`` where the finder would find
    nothing (``c21cm_dexm_is_empty``)."""
    lib = load()
    lib.c21cm_dexm_ladder.restype = C.c_int
    lib.c21cm_dexm_ladder.argtypes = [C.c_double, C.c_void_p]
    spec = S.FindHalosSpec()
    check(lib.c21cm_dexm_ladder(float(redshift), C.byref(spec)), "c21cm_dexm_ladder")
    spec.seed = int(seed)
    return spec


def find_halos(spec: S.FindHalosSpec, hires_density, out: S.HaloCatalogStruct, filtered=None, in_halo=None,
               overlap=None, stream=None):
    """The DexM halo finder on the MI355X (reference: HaloCatalog.c:38-456): ``hires_density`` [DIM^3] (the
    z = 0 field) filtered on the ladder of ``spec``, every rung's candidates decided as the reference's
    serial raster scan decides them, the halos appended to ``out`` (structs.empty_halo_catalog) in raster
    order.  ``in_halo`` [DIM^3] uint8 receives the mask, ``overlap`` [HII_DIM^3] (needed when
    ``spec.hii_dim > 0``) the covered fraction of every low-resolution cell; ``filtered`` [n_R, DIM^3] is the
    test hook of ``spec.filtered_mode``.  Arrays are numpy or torch CUDA tensors.  Returns ``out``."""
    lib = load()
    lib.c21cm_find_halos_grids.restype = C.c_int
    lib.c21cm_find_halos_grids.argtypes = [C.c_void_p] * 7
    n = spec.dim * spec.dim * spec.dim_z
    for name, a, size, width in (("hires_density", hires_density, n, 4), ("filtered", filtered, spec.n_R * n, 4),
                                 ("in_halo", in_halo, n, 1),
                                 ("overlap", overlap, spec.hii_dim * spec.hii_dim * spec.hii_dim_z, 4)):
        if a is None:
            continue
        count = a.numel() if _is_torch(a) else a.size
        itemsize = a.element_size() if _is_torch(a) else a.itemsize
        contiguous = a.is_contiguous() if _is_torch(a) else a.flags["C_CONTIGUOUS"]
        if count != size or itemsize != width or not contiguous:
            raise ValueError(f"find_halos: {name} must be contiguous, {size} elements of {width} byte(s)")
    check(lib.c21cm_find_halos_grids(C.byref(spec), _vptr(hires_density), _vptr(filtered), C.byref(out),
                                     _vptr(in_halo), _vptr(overlap), _stream(stream)), "c21cm_find_halos_grids")
    return out


def find_halos_report() -> S.FindHalosReport:
    """Per rung of the last ``find_halos`` call: candidates, accepted halos, rounds, serial tail."""
    lib = load()
    lib.c21cm_find_halos_last_report.restype = None
    lib.c21cm_find_halos_last_report.argtypes = [C.c_void_p]
    rep = S.FindHalosReport()
    lib.c21cm_find_halos_last_report(C.byref(rep))
    return rep


def perturb_halos_grids(spec: S.PerturbHalosSpec, consts: S.HaloConsts, ics: dict,
                        catalog: S.HaloCatalogStruct, out: S.PerturbedHaloCatalogStruct,
                        log10_mturn_acg=None, log10_mturn_mcg=None, stream=None):
    """ComputePerturbedHaloCatalog with explicit scalars on the MI355X (reference:
    PerturbedHaloCatalog.c:25-149, HaloBox.c:781-880): the halos of ``catalog`` displaced with the
    velocity grids of ``ics`` and converted to galaxy properties into the arrays of ``out``
    (structs.perturbed_halo_catalog, or any PerturbedHaloCatalogStruct; NULL optional arrays are
    skipped).  The turnover grids are read with ``consts.use_mini_halos``.  Returns ``out``."""
    lib = load(require_gpu=True)
    lib.c21cm_perturb_halos_grids.restype = C.c_int
    lib.c21cm_perturb_halos_grids.argtypes = [C.c_void_p] * 3 + [S.c_float_p] * 2 + [C.c_void_p] * 3
    icss = ics_struct(ics)
    check(lib.c21cm_perturb_halos_grids(C.byref(spec), C.byref(consts), C.byref(icss),
                                        _fptr(log10_mturn_acg), _fptr(log10_mturn_mcg),
                                        C.byref(catalog), C.byref(out), _stream(stream)),
          "c21cm_perturb_halos_grids")
    return out


def halobox_turnovers(spec: S.MturnSpec, m_turn, below_z_heat_max, n_threads, prev_G12,
                      prev_z_reion, J_21_LW, vcb=None, like=None, stream=None):
    """get_log10_turnovers (HaloBox.c:465-516) on the MI355X: (log10 M_turn,a, log10 M_turn,m,
    (<a>, <m>)); grids allocated like ``like`` (default: ``J_21_LW``)."""
    ref = J_21_LW if like is None else like
    a, m = _new_like(ref, 0.0), _new_like(ref, 0.0)
    ave = (C.c_double * 2)()
    lib = load()
    lib.c21cm_halobox_turnovers.restype = C.c_int
    lib.c21cm_halobox_turnovers.argtypes = [C.POINTER(S.MturnSpec), C.c_double, C.c_int, C.c_int] + [
        C.c_void_p] * 6 + [C.POINTER(C.c_double), C.c_void_p]
    check(lib.c21cm_halobox_turnovers(C.byref(spec), float(m_turn), int(below_z_heat_max),
                                      int(n_threads), _vptr(prev_G12), _vptr(prev_z_reion),
                                      _vptr(J_21_LW), _vptr(vcb), _vptr(a), _vptr(m), ave,
                                      _stream(stream)), "c21cm_halobox_turnovers")
    return a, m, (ave[0], ave[1])


def fill_Rbox_grids(spec: S.RboxSpec, field, stream=None) -> dict:
    """prepare_filter_boxes + fill_Rbox_table on the MI355X (reference:
    src/py21cmfast/src/SpinTemperatureBox.c:502-520,560-636).  Returns dict(result [n_R, ...],
    min, average, max [n_R]); result lives where ``field`` lives."""
    n_R = spec.n_R
    shape = (n_R,) + tuple(field.shape)
    if _is_torch(field):
        import torch

        result = torch.zeros(shape, dtype=torch.float32, device=field.device)
    else:
        result = np.zeros(shape, np.float32)
    mn, av, mx = ((C.c_double * n_R)() for _ in range(3))
    check(load().c21cm_fill_Rbox_grids(C.byref(spec), _vptr(field), _vptr(result), mn, av, mx,
                                       _stream(stream)), "c21cm_fill_Rbox_grids")
    return {"result": result, "min": np.array(mn[:]), "average": np.array(av[:]),
            "max": np.array(mx[:])}


def annular_filter_grids(spec: S.AnnularSpec, inputs, stream=None) -> dict:
    """one_annular_filter for ``spec.n_grids`` grids of one shell on the MI355X (reference:
    src/py21cmfast/src/SpinTemperatureBox.c:642-742).  Returns dict(outputs [list], u_avg, f_avg)."""
    n = spec.n_grids
    assert len(inputs) == n
    outputs = [_new_like(a, 0.0) for a in inputs]
    in_p = (C.c_void_p * n)(*[_vptr(a).value if _is_torch(a) else a.ctypes.data for a in inputs])
    out_p = (C.c_void_p * n)(*[_vptr(a).value if _is_torch(a) else a.ctypes.data for a in outputs])
    u, f = (C.c_double * n)(), (C.c_double * n)()
    check(load().c21cm_annular_filter_grids(C.byref(spec), in_p, out_p, u, f, _stream(stream)),
          "c21cm_annular_filter_grids")
    return {"outputs": outputs, "u_avg": np.array(u[:]), "f_avg": np.array(f[:])}


TS_FIELDS = ("spin_temperature", "kinetic_temp_neutral", "xray_ionised_fraction")


def ts_grids(spec: S.TsSpec, density, previous: dict, source: dict | None = None,
             filtered_density=None, stream=None) -> dict:
    """The per-cell part of ComputeTsBox on the MI355X (reference:
    src/py21cmfast/src/SpinTemperatureBox.c:1387-1946 from the first cell loop on): the R loop
    over the source grids (``source``: filtered_sfr / filtered_xray [n_step, ...], Lagrangian
    models) or over the filtered densities (``filtered_density`` [n_step, ...] with the spec's
    SFRD tables), then the x_e / T_k update and T_s of every cell.  ``previous``: the three boxes
    of the previous snapshot.  Outputs live where ``density`` lives; ``report`` holds box means.
    With ``spec.use_mini_halos`` (2-D tables and ``spec.filtered_log10_mcrit`` set by the caller)
    the result also holds ``J_21_LW``."""
    out = {k: _new_like(density, 0.0) for k in TS_FIELDS}
    prev = S.TsBoxStruct(**{k: _fptr(previous[k]) for k in TS_FIELDS})
    box = S.TsBoxStruct(**{k: _fptr(out[k]) for k in TS_FIELDS})
    if spec.use_mini_halos:
        out["J_21_LW"] = _new_like(density, 0.0)
        box.J_21_LW = _fptr(out["J_21_LW"])
    src = S.XraySourceBoxStruct(**{k: _fptr(v) for k, v in (source or {}).items()})
    rep = S.TsReport()
    check(load().c21cm_ts_grids(C.byref(spec), _vptr(density), C.byref(prev), C.byref(src),
                                _vptr(filtered_density), C.byref(box), C.byref(rep),
                                _stream(stream)), "c21cm_ts_grids")
    out["report"] = rep
    return out


def ts_shell_sums(spec: S.TsSpec, density, previous: dict, source: dict | None = None,
                  filtered_density=None, stream=None):
    """The shell loop of ``ts_grids`` alone (``c21cm_ts_shell_sums``): the six per-cell sums over the
    spec's shells as a device float64 tensor [6, N] (heat, ion, lya, starlya, cont, inj).  The tensor
    starts as NaN, so rows the loop does not write stay visible: row 0 is written as zero without
    ``use_xray_heating``, rows 4 and 5 are untouched without ``use_lya_heating``.  Arrays may be numpy
    or CUDA tensors; no mini-halos, and not before the first sources (``no_light``)."""
    import torch

    dev = density.device if _is_torch(density) else "cuda"
    sums = torch.full((6, int(np.prod(density.shape))), float("nan"), dtype=torch.float64, device=dev)
    prev = S.TsBoxStruct(**{k: _fptr(previous[k]) for k in TS_FIELDS})
    src = S.XraySourceBoxStruct(**{k: _fptr(v) for k, v in (source or {}).items()})
    lib = load()
    lib.c21cm_ts_shell_sums.restype = C.c_int
    lib.c21cm_ts_shell_sums.argtypes = [C.c_void_p] * 7
    check(lib.c21cm_ts_shell_sums(C.byref(spec), _vptr(density), C.byref(prev), C.byref(src),
                                  _vptr(filtered_density), C.c_void_p(sums.data_ptr()),
                                  _stream(stream)), "c21cm_ts_shell_sums")
    return sums


def ts_last_route() -> dict:
    """What the spin-temperature launchers chose in the last call (``c21hip_ts_last_route``): ``loop``
    (shell-loop version 1, 2, 3), ``cells`` per thread (1, 2), ``mode`` (0 Lagrangian grids, 1 ln SFRD
    tables, 2 dfcoll/dz tables) and ``box_sum`` (None with Lagrangian grids, else "scalar", "float4" or
    "sfrd_sum2")."""
    lib = load()
    lib.c21hip_ts_last_route.restype = C.c_int
    lib.c21hip_ts_last_route.argtypes = []
    r = lib.c21hip_ts_last_route()
    return {"loop": r & 3, "cells": (r >> 2) & 3, "mode": (r >> 4) & 3,
            "box_sum": (None, "scalar", "float4", "sfrd_sum2")[(r >> 6) & 3]}


def ts_mcrit_grid(spec: S.MturnSpec, m_turn: float, J_21_LW, vcb=None, stream=None):
    """log10 of the Lyman-Werner turnover mass per cell from the previous TsBox's J_21_LW
    (prepare_filter_boxes, SpinTemperatureBox.c:535-565); allocated like ``J_21_LW``."""
    out = _new_like(J_21_LW, 0.0)
    lib = load()
    lib.c21cm_ts_mcrit_grid.restype = C.c_int
    lib.c21cm_ts_mcrit_grid.argtypes = [C.POINTER(S.MturnSpec), C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    check(lib.c21cm_ts_mcrit_grid(C.byref(spec), float(m_turn), _vptr(J_21_LW), _vptr(vcb),
                                  _vptr(out), _stream(stream)), "c21cm_ts_mcrit_grid")
    return out


def ts_first_grids(spec: S.TsFirstSpec, density, stream=None) -> dict:
    """init_first_Ts (SpinTemperatureBox.c:892-927) on the MI355X."""
    out = {k: _new_like(density, 0.0) for k in TS_FIELDS}
    box = S.TsBoxStruct(**{k: _fptr(out[k]) for k in TS_FIELDS})
    check(load().c21cm_ts_first_grids(C.byref(spec), _vptr(density), C.byref(box), _stream(stream)),
          "c21cm_ts_first_grids")
    return out


LC_MAX_FIELDS = 16  # C21CM_LC_MAX_FIELDS


def _f32_dense(a, what):
    ok = (a.is_contiguous() and str(a.dtype) == "torch.float32") if _is_torch(a) else (
        a.dtype == np.float32 and a.flags["C_CONTIGUOUS"])
    if not ok:
        raise ValueError(f"{what} must be a C-contiguous float32 array")


def lightcone_slices(lightcones: dict, box_lo: dict, box_hi: dict, i0: int, plane, w_lo, w_hi,
                     w_norm: float, mean_max=("z_reion",), stream=None):
    """Fill slices [i0, i0 + len(plane)) of every lightcone in ``lightcones`` (name -> array of shape
    (HII_DIM, HII_DIM, n_slices)) from the node boxes ``box_lo[name]`` / ``box_hi[name]`` (shape
    (HII_DIM, HII_DIM, HII_D_PARA)) that bracket them (reference: lightconers.py:162-319):
    (w_lo box_lo + w_hi box_hi) / w_norm at plane ``plane[j]`` of the boxes, fp64, stored as fp32;
    fields named in ``mean_max`` take the larger value where the two boxes differ in sign.  The
    tables come from ``drivers.RectilinearLightconer.slab_tables``.  Arrays may be numpy or torch CUDA
    tensors, mixed freely; a numpy lightcone receives only the slices of this call."""
    plane = np.ascontiguousarray(plane, np.int32)
    w_lo = np.ascontiguousarray(w_lo, np.float64)
    w_hi = np.ascontiguousarray(w_hi, np.float64)
    run = len(plane)
    if len(w_lo) != run or len(w_hi) != run:
        raise ValueError("plane, w_lo and w_hi must have the same length")
    names = list(lightcones)
    if not names:
        raise ValueError("no lightcone to fill")
    first = lightcones[names[0]]
    n, _, n_slices = (int(x) for x in first.shape)
    d_para = int(box_lo[names[0]].shape[-1])
    for k in names:
        if tuple(lightcones[k].shape) != (n, n, n_slices):
            raise ValueError(f"lightcone {k!r} has shape {tuple(lightcones[k].shape)}")
        _f32_dense(lightcones[k], f"lightcone {k!r}")
        for b in (box_lo[k], box_hi[k]):
            _f32_dense(b, f"node box of {k!r}")
            if tuple(b.shape) != (n, n, d_para):
                raise ValueError(f"node box of {k!r} has shape {tuple(b.shape)}, not {(n, n, d_para)}")
    lib = load()
    lib.c21cm_lightcone_slab_grids.restype = C.c_int
    for c0 in range(0, len(names), LC_MAX_FIELDS):
        chunk = names[c0:c0 + LC_MAX_FIELDS]
        ptrs = [(C.c_void_p * len(chunk))(*[_vptr(d[k]).value for k in chunk])
                for d in (box_lo, box_hi, lightcones)]
        spec = S.LightconeSpec(
            hii_dim=n, hii_d_para=d_para, n_slices=n_slices, i0=int(i0), i1=int(i0) + run,
            n_fields=len(chunk), mean_max=sum(1 << q for q, k in enumerate(chunk) if k in mean_max),
            plane=plane.ctypes.data_as(C.POINTER(C.c_int)), w_lo=w_lo.ctypes.data_as(S.c_double_p),
            w_hi=w_hi.ctypes.data_as(S.c_double_p), w_norm=float(w_norm))
        check(lib.c21cm_lightcone_slab_grids(C.byref(spec), *ptrs, _stream(stream)),
              "c21cm_lightcone_slab_grids")


def lightcone_dvdr(brightness_temp, los_velocity, hubble, dx: float, max_dvdr: float, tau_21=None,
                   stream=None):
    """Correct a brightness-temperature lightcone in place for the line-of-sight velocity gradient
    (reference: rsds.py:16-103 with periodic = False).  The line of sight is the last axis: a rectilinear
    lightcone (HII_DIM, HII_DIM, n_slices) or an angular one (n_pix, n_slices).  ``hubble``: H(z) [1/s] of every slice;
    ``tau_21`` given: the USE_TS_FLUCT form, else the Taylor form clipped at +-max_dvdr H."""
    shape = tuple(int(x) for x in brightness_temp.shape)
    if len(shape) < 1:
        raise ValueError("brightness_temp must have a line-of-sight axis")
    n_slices = shape[-1]
    # (HII_DIM, HII_DIM, n_slices): the rectilinear entry; any other (..., n_slices): the column entry
    square = len(shape) == 3 and shape[0] == shape[1]
    for a in (brightness_temp, los_velocity, tau_21):
        if a is not None:
            _f32_dense(a, "brightness_temp / los_velocity / tau_21")
        if a is not None and tuple(a.shape) != shape:
            raise ValueError("los_velocity / tau_21 must have the shape of brightness_temp")
    hubble = np.ascontiguousarray(hubble, np.float64)
    if hubble.shape != (n_slices,):
        raise ValueError(f"hubble must hold one H(z) per slice ({n_slices})")
    spec = S.DvdrSpec(hii_dim=shape[0] if square else 0, n_slices=n_slices, dx=float(dx), max_dvdr=float(max_dvdr),
                      use_ts_fluct=int(tau_21 is not None), hubble=hubble.ctypes.data_as(S.c_double_p))
    lib = load()
    ptrs = (_vptr(brightness_temp), _vptr(los_velocity), _vptr(tau_21), _stream(stream))
    if square:
        lib.c21cm_lightcone_dvdr_grids.restype = C.c_int
        check(lib.c21cm_lightcone_dvdr_grids(C.byref(spec), *ptrs), "c21cm_lightcone_dvdr_grids")
    else:
        lib.c21cm_lightcone_dvdr_columns_grids.restype = C.c_int
        n_cols = int(np.prod(shape[:-1], dtype=np.int64))
        check(lib.c21cm_lightcone_dvdr_columns_grids(C.byref(spec), C.c_longlong(n_cols), *ptrs),
              "c21cm_lightcone_dvdr_columns_grids")


DVDR_PERIODIC_METHODS = {"auto": 0, "fft": 1, "direct": 2}


def dvdr_periodic(brightness_temp, los_velocity, hubble, dx: float, max_dvdr: float, tau_21=None,
                  method: str = "auto", out=None, lib=None, stream=None):
    """The brightness temperature of a coeval box corrected for the line-of-sight velocity gradient, the line
    of sight (the last axis) periodic (reference: rsds.py:16-103 with periodic = True).  The gradient is
    ``irfft(1j k rfft(los_velocity))`` along the last axis, ``k = 2 pi rfftfreq(n, dx)``; ``hubble``: H(z)
    [1/s], a scalar or one per slice; ``tau_21`` given: the USE_TS_FLUCT form, else the Taylor form clipped at
    +-max_dvdr H.  ``method``: "auto" (the fp32 line transform for n = 2^k, 8 .. 1024, else the exact circulant
    sum, n <= 1536), "fft" or "direct".  Arrays are float32, 2-D ``(n_cols, n)`` or 3-D, numpy or torch CUDA
    tensors; returns ``out`` (default: a new array where ``brightness_temp`` lives), which may be
    ``brightness_temp`` itself.  No other input is written."""
    shape = tuple(int(x) for x in brightness_temp.shape)
    if len(shape) not in (2, 3):
        raise ValueError("brightness_temp must be a 2-D (n_cols, n) or 3-D (n, n, n_slices) array")
    if method not in DVDR_PERIODIC_METHODS:
        raise ValueError(f"method must be one of {sorted(DVDR_PERIODIC_METHODS)}")
    n_slices = shape[-1]
    # what the kernels take (csrc/hip/dvdr_periodic_kernels.hip); the library checks the same
    pow2 = 8 <= n_slices <= 1024 and n_slices & (n_slices - 1) == 0
    if n_slices < 2:
        raise ValueError("a periodic line of sight needs at least 2 slices")
    if method == "fft" and not pow2:
        raise ValueError(f"method 'fft' takes a line of 2^k cells, 8 <= n <= 1024, not {n_slices}")
    if (method == "direct" or not pow2) and n_slices > 1536:
        raise ValueError(f"the direct sum takes a line of at most 1536 cells, not {n_slices}")
    if out is None:
        out = _new_like(brightness_temp, 0.0)
    for a in (brightness_temp, los_velocity, tau_21, out):
        if a is not None:
            _f32_dense(a, "brightness_temp / los_velocity / tau_21 / out")
        if a is not None and tuple(a.shape) != shape:
            raise ValueError("los_velocity / tau_21 / out must have the shape of brightness_temp")
    hubble = np.ascontiguousarray(np.broadcast_to(np.asarray(hubble, np.float64), (n_slices,)))
    spec = S.DvdrPeriodicSpec(n_cols=int(np.prod(shape[:-1], dtype=np.int64)), n_slices=n_slices, dx=float(dx),
                              max_dvdr=float(max_dvdr), use_ts_fluct=int(tau_21 is not None),
                              method=DVDR_PERIODIC_METHODS[method], hubble=hubble.ctypes.data_as(S.c_double_p))
    lib = lib or load()
    lib.c21cm_dvdr_periodic_grids.restype = C.c_int
    check(lib.c21cm_dvdr_periodic_grids(C.byref(spec), _vptr(brightness_temp), _vptr(los_velocity),
                                        _vptr(tau_21), _vptr(out), _stream(stream)),
          "c21cm_dvdr_periodic_grids")
    return out


def rsd_shift(fields, los_velocity, disp_scale, n_sub: int = 4, periodic: bool = False, out=None,
              stream=None):
    """Move every cell of each array in ``fields`` along the last axis by ``los_velocity *
    disp_scale[j]`` pixels (reference: rsds.py:184-255 rsds_shift): the displacement is interpolated
    linearly onto ``n_sub`` sub-cells per slice, each sub-cell is deposited by linear cloud-in-cell and
    the sub-cells are summed back; ``periodic`` wraps the line of sight, else what leaves it is lost.
    ``fields``: a dict (name -> array) or a sequence of float32 arrays of the shape of ``los_velocity``
    (..., n_slices); ``disp_scale``: pixels per unit of velocity, one per slice.  ``out`` (same kind
    as ``fields``; default: new arrays where each field lives) may be ``fields`` itself.  Arrays may
    be numpy or torch CUDA tensors, mixed freely; returns ``out``."""
    named = isinstance(fields, dict)
    names = list(fields) if named else list(range(len(fields)))
    if not names:
        raise ValueError("no field to shift")
    shape = tuple(int(x) for x in los_velocity.shape)
    if len(shape) < 1:
        raise ValueError("los_velocity must have a line-of-sight axis")
    n_slices = shape[-1]
    n_cols = int(np.prod(shape[:-1], dtype=np.int64))
    _f32_dense(los_velocity, "los_velocity")
    if out is None:
        made = {k: _new_like(fields[k], 0.0) for k in names}
        out = made if named else [made[k] for k in names]
    for k in names:
        for a, what in ((fields[k], "field"), (out[k], "output")):
            _f32_dense(a, f"{what} {k!r}")
            if tuple(a.shape) != shape:
                raise ValueError(f"{what} {k!r} has shape {tuple(a.shape)}, not that of los_velocity {shape}")
    disp_scale = np.ascontiguousarray(np.broadcast_to(np.asarray(disp_scale, np.float64), (n_slices,)))
    spec = S.RsdSpec(n_cols=n_cols, n_slices=n_slices, n_fields=len(names), n_sub=int(n_sub),
                     periodic=int(bool(periodic)), disp_scale=disp_scale.ctypes.data_as(S.c_double_p))
    ins = (C.c_void_p * len(names))(*[_vptr(fields[k]).value for k in names])
    outs = (C.c_void_p * len(names))(*[_vptr(out[k]).value for k in names])
    lib = load()
    lib.c21cm_rsd_shift_grids.restype = C.c_int
    check(lib.c21cm_rsd_shift_grids(C.byref(spec), ins, outs, _vptr(los_velocity), _stream(stream)),
          "c21cm_rsd_shift_grids")
    return out


def _f64_dense(a, what):
    ok = (a.is_contiguous() and str(a.dtype) == "torch.float64") if _is_torch(a) else (
        a.dtype == np.float64 and a.flags["C_CONTIGUOUS"])
    if not ok:
        raise ValueError(f"{what} must be a C-contiguous float64 array")


def lightcone_angular(lightcones: dict, box_lo: dict, box_hi: dict, i0: int, distance, w_lo, w_hi,
                      w_norm: float, nhat, origin=(0.0, 0.0, 0.0), order: int = 1, mean_max=("z_reion",),
                      stream=None):
    """Fill slices [i0, i0 + len(distance)) of every angular lightcone in ``lightcones`` (name -> array of
    shape (n_pix, n_slices)) from the node boxes ``box_lo[name]`` / ``box_hi[name]`` (shape (HII_DIM,
    HII_DIM, HII_D_PARA), periodic) that bracket them (reference: lightconers.py:162-287 with the
    AngularLightconer).  Pixel p of slice j sits at ``distance[j] * nhat[:, p] + origin``
    (cells); its value is the B-spline interpolation of ``order`` (0, 1, 3, 5) there, every tap
    redshift-interpolated first, (w_lo box_lo + w_hi box_hi) / w_norm in fp64 (``mean_max`` fields: the
    larger value where the two differ in sign).  For orders 3 and 5 the boxes must be B-spline
    coefficients (``spline_prefilter``).  A vector field (``los_velocity``) gives a triple of boxes
    (x, y, z components) and stores their projection on ``nhat``.  ``nhat``: float64 (3, n_pix), best a
    torch CUDA tensor made once per run.  Arrays may be numpy or torch CUDA tensors, mixed freely; a numpy
    lightcone receives only the slices of this call.  The tables come from
    ``drivers.AngularLightconer.angular_tables``."""
    distance = np.ascontiguousarray(distance, np.float64)
    w_lo = np.ascontiguousarray(w_lo, np.float64)
    w_hi = np.ascontiguousarray(w_hi, np.float64)
    run = len(distance)
    if len(w_lo) != run or len(w_hi) != run:
        raise ValueError("distance, w_lo and w_hi must have the same length")
    if int(order) not in (0, 1, 3, 5):
        raise ValueError("order must be 0, 1, 3 or 5")
    names = list(lightcones)
    if not names:
        raise ValueError("no lightcone to fill")
    n_pix, n_slices = (int(x) for x in lightcones[names[0]].shape)
    _f64_dense(nhat, "nhat")
    if tuple(nhat.shape) != (3, n_pix):
        raise ValueError(f"nhat must have shape (3, {n_pix})")
    origin = np.asarray(origin, np.float64)
    if origin.shape != (3,):
        raise ValueError("origin must hold three coordinates")

    def boxes(d, k):
        v = d[k]
        return list(v) if isinstance(v, (tuple, list)) else [v]

    box_shape = None
    for k in names:
        if tuple(lightcones[k].shape) != (n_pix, n_slices):
            raise ValueError(f"lightcone {k!r} has shape {tuple(lightcones[k].shape)}")
        _f32_dense(lightcones[k], f"lightcone {k!r}")
        lo, hi = boxes(box_lo, k), boxes(box_hi, k)
        if len(lo) not in (1, 3) or len(hi) != len(lo):
            raise ValueError(f"{k!r}: one node box, or three components of a vector field, on both sides")
        for b in lo + hi:
            _f32_dense(b, f"node box of {k!r}")
            box_shape = box_shape or tuple(int(x) for x in b.shape)
            if len(box_shape) != 3 or box_shape[0] != box_shape[1] or tuple(b.shape) != box_shape:
                raise ValueError(f"node box of {k!r} has shape {tuple(b.shape)}: (HII_DIM, HII_DIM, HII_D_PARA)"
                                 " and the same for every field")
    nhat_p = C.cast(_vptr(nhat), S.c_double_p)
    lib = load()
    lib.c21cm_lightcone_angular_grids.restype = C.c_int
    for c0 in range(0, len(names), LC_MAX_FIELDS):
        chunk = names[c0:c0 + LC_MAX_FIELDS]
        lo = [b for k in chunk for b in boxes(box_lo, k)]
        hi = [b for k in chunk for b in boxes(box_hi, k)]
        ptrs = [(C.c_void_p * len(v))(*[_vptr(a).value for a in v]) for v in (lo, hi)]
        outs = (C.c_void_p * len(chunk))(*[_vptr(lightcones[k]).value for k in chunk])
        spec = S.AngularSpec(
            hii_dim=box_shape[0], hii_d_para=box_shape[2], n_pix=n_pix, n_slices=n_slices, i0=int(i0),
            i1=int(i0) + run, n_fields=len(chunk),
            mean_max=sum(1 << q for q, k in enumerate(chunk) if k in mean_max),
            vector=sum(1 << q for q, k in enumerate(chunk) if len(boxes(box_lo, k)) == 3), order=int(order),
            nhat=nhat_p, origin=(C.c_double * 3)(*origin), distance=distance.ctypes.data_as(S.c_double_p),
            w_lo=w_lo.ctypes.data_as(S.c_double_p), w_hi=w_hi.ctypes.data_as(S.c_double_p), w_norm=float(w_norm))
        check(lib.c21cm_lightcone_angular_grids(C.byref(spec), *ptrs, outs, _stream(stream)),
              "c21cm_lightcone_angular_grids")


def spline_prefilter(boxes, order: int, out=None, stream=None):
    """B-spline coefficients of ``order`` (3 or 5) of periodic 3-D boxes: what
    ``scipy.ndimage.spline_filter(box, order, mode="grid-wrap")`` computes, stored as float32.  ``boxes``: a
    dict (name -> array) or a sequence of float32 arrays of one shape; ``out`` (same kind; default: new
    arrays where each box lives) may be ``boxes`` itself.  Arrays may be numpy or torch CUDA tensors,
    mixed freely; returns ``out``."""
    named = isinstance(boxes, dict)
    names = list(boxes) if named else list(range(len(boxes)))
    if not names:
        raise ValueError("no box to prefilter")
    shape = tuple(int(x) for x in boxes[names[0]].shape)
    if len(shape) != 3:
        raise ValueError("the boxes must be 3-D")
    if out is None:
        made = {k: _new_like(boxes[k], 0.0) for k in names}
        out = made if named else [made[k] for k in names]
    for k in names:
        for a, what in ((boxes[k], "box"), (out[k], "output")):
            _f32_dense(a, f"{what} {k!r}")
            if tuple(a.shape) != shape:
                raise ValueError(f"{what} {k!r} has shape {tuple(a.shape)}, not {shape}")
    ins = (C.c_void_p * len(names))(*[_vptr(boxes[k]).value for k in names])
    outs = (C.c_void_p * len(names))(*[_vptr(out[k]).value for k in names])
    lib = load()
    lib.c21cm_spline_prefilter_grids.restype = C.c_int
    check(lib.c21cm_spline_prefilter_grids(*shape, int(order), len(names), ins, outs, _stream(stream)),
          "c21cm_spline_prefilter_grids")
    return out


def power_spectrum(field, field2, shape, lengths, edges, edges_par=None, *, offsets=(0,), row_pitch=None,
                   ignore_zero_mode=False, ignore_kperp_zero=False, ignore_kpar_zero=False, windows=None,
                   inv_mean_w2=1.0, mu_range=None, wedge=None, want_variance=False, entry=None, stream=None):
    """Binned power spectra of ``len(offsets)`` boxes of ``shape`` = (nx, ny, nz) cells and ``lengths``
    (Lx, Ly, Lz) read from the float32 array ``field`` (box b at flat element ``offsets[b] + (i ny + j)
    row_pitch + l``; ``row_pitch`` defaults to nz), cross spectra with ``field2`` (same layout) when given.
    ``edges``: the |k| edges, or the k_perp edges with ``edges_par`` the k_par edges (cylindrical).
    Returns ``(power, kmean, counts)``: float64, float64, int64, shaped (n_batch, n_bins) or (n_batch,
    n_perp, n_par) with kmean (n_batch, n_perp + n_par); numpy for numpy input, torch on the field's device
    for a torch CUDA field.

    The options of ``c21cm_power_opts``: ``windows`` = (wx, wy, wz), each None or float64 weights of that axis,
    with ``inv_mean_w2`` = 1 / <W^2>; ``mu_range`` = (mu_min, mu_max); ``wedge`` = (slope, buffer);
    ``want_variance`` appends the per-bin variance (shaped as power) to the result.  ``entry``: None takes
    ``c21cm_power_spectrum_grids`` when every option is off and ``c21cm_power_spectrum_ex_grids`` otherwise;
    "ex" forces the latter with the options struct, "ex-null" with ``opts = NULL``."""
    if entry not in (None, "ex", "ex-null"):
        raise ValueError(f"unknown entry {entry!r}")
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    size = int(np.prod(field.shape, dtype=np.int64))
    for a, what in ((field, "field"), (field2, "field2")):
        if a is None:
            continue
        _f32_dense(a, what)
        if int(np.prod(a.shape, dtype=np.int64)) != size:
            raise ValueError(f"{what} has {int(np.prod(a.shape))} elements, not {size}")
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    edges = np.ascontiguousarray(edges, np.float64)
    cyl = edges_par is not None
    edges_par = np.ascontiguousarray(edges_par if cyl else [0.0, 1.0], np.float64)
    bins = S.PowerBins(cylindrical=int(cyl), n_bins=len(edges) - 1, n_bins_par=len(edges_par) - 1,
                       edges=edges.ctypes.data_as(S.c_double_p), edges_par=edges_par.ctypes.data_as(S.c_double_p),
                       ignore_zero_mode=int(bool(ignore_zero_mode)), ignore_kperp_zero=int(bool(ignore_kperp_zero)),
                       ignore_kpar_zero=int(bool(ignore_kpar_zero)))
    nb, npar = len(edges) - 1, len(edges_par) - 1
    pshape = (n_batch, nb, npar) if cyl else (n_batch, nb)
    kshape = (n_batch, nb + npar) if cyl else (n_batch, nb)
    if _is_torch(field):
        import torch

        power = torch.empty(pshape, dtype=torch.float64, device=field.device)
        kmean = torch.empty(kshape, dtype=torch.float64, device=field.device)
        counts = torch.empty(pshape, dtype=torch.int64, device=field.device)
        variance = torch.empty(pshape, dtype=torch.float64, device=field.device) if want_variance else None
    else:
        power, kmean, counts = np.empty(pshape), np.empty(kshape), np.empty(pshape, np.int64)
        variance = np.empty(pshape) if want_variance else None
    Lx, Ly, Lz = (float(x) for x in lengths)
    any_opt = windows is not None or mu_range is not None or wedge is not None or want_variance
    if entry == "ex-null" and any_opt:
        raise ValueError("entry='ex-null' carries no options")
    if any_opt or entry is not None:
        wins = [None if w is None else np.ascontiguousarray(w, np.float64) for w in (windows or (None,) * 3)]
        for w, n, ax in zip(wins, (nx, ny, nz), "xyz"):
            if w is not None and w.shape != (n,):
                raise ValueError(f"the {ax} window must hold {n} weights")
        opts = S.PowerOpts(
            window_x=None if wins[0] is None else wins[0].ctypes.data_as(S.c_double_p),
            window_y=None if wins[1] is None else wins[1].ctypes.data_as(S.c_double_p),
            window_z=None if wins[2] is None else wins[2].ctypes.data_as(S.c_double_p),
            inv_mean_w2=float(inv_mean_w2),
            mu_min_sq=0.0 if mu_range is None else float(mu_range[0]) * float(mu_range[0]),
            mu_max_sq=1.0 if mu_range is None else float(mu_range[1]) * float(mu_range[1]),
            use_mu=int(mu_range is not None),
            wedge_slope_sq=0.0 if wedge is None else float(wedge[0]) * float(wedge[0]),
            wedge_buffer=0.0 if wedge is None else float(wedge[1]), use_wedge=int(wedge is not None),
            want_variance=int(bool(want_variance)))
        lib = load()
        lib.c21cm_power_spectrum_ex_grids.restype = C.c_int
        lib.c21cm_power_spectrum_ex_grids.argtypes = [
            C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_double,
            C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p]
        check(lib.c21cm_power_spectrum_ex_grids(
            _vptr(field), _vptr(field2), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p), Lx, Ly,
            Lz, C.byref(bins), None if entry == "ex-null" else C.byref(opts), _vptr(power), _vptr(kmean),
            _vptr(variance), _vptr(counts), _stream(stream)), "c21cm_power_spectrum_ex_grids")
        return (power, kmean, counts, variance) if want_variance else (power, kmean, counts)
    lib = load()
    lib.c21cm_power_spectrum_grids.restype = C.c_int
    lib.c21cm_power_spectrum_grids.argtypes = [
        C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_double,
        C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(lib.c21cm_power_spectrum_grids(_vptr(field), _vptr(field2), nx, ny, nz, n_batch, row_pitch,
                                         offsets.ctypes.data_as(C.c_void_p), Lx, Ly, Lz, C.byref(bins),
                                         _vptr(power), _vptr(kmean), _vptr(counts), _stream(stream)),
          "c21cm_power_spectrum_grids")
    return power, kmean, counts


def field_moments(field, shape, *, offsets=(0,), row_pitch=None, edges=None, stream=None):
    """One-point statistics of ``len(offsets)`` boxes of ``shape`` = (nx, ny, nz) cells read from the float32
    array ``field`` (the layout of ``power_spectrum``): ``(moments, hist)`` with moments float64 (n_batch, 4) =
    mean, m2, m3, m4 (m_p = sum (v - mean)^p / N) and, with ``edges`` (n_bins + 1, increasing), hist int64
    (n_batch, n_bins) = the cells per half-open bin as ``np.digitize``; hist is None without edges.  numpy for
    numpy input, torch on the field's device for a torch CUDA field."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    n_bins = 0
    if edges is not None:
        edges = np.ascontiguousarray(edges, np.float64)
        if edges.ndim != 1 or edges.size < 2:
            raise ValueError("edges must be a 1-D array of at least 2 values")
        n_bins = len(edges) - 1
    hist = None
    if _is_torch(field):
        import torch

        moments = torch.empty((n_batch, 4), dtype=torch.float64, device=field.device)
        if n_bins:
            hist = torch.empty((n_batch, n_bins), dtype=torch.int64, device=field.device)
    else:
        moments = np.empty((n_batch, 4))
        if n_bins:
            hist = np.empty((n_batch, n_bins), np.int64)
    lib = load()
    lib.c21cm_field_moments_grids.restype = C.c_int
    lib.c21cm_field_moments_grids.argtypes = [
        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
        C.c_void_p, C.c_void_p]
    check(lib.c21cm_field_moments_grids(_vptr(field), nx, ny, nz, n_batch, row_pitch,
                                        offsets.ctypes.data_as(C.c_void_p), n_bins,
                                        None if edges is None else edges.ctypes.data_as(C.c_void_p), _vptr(moments),
                                        _vptr(hist), _stream(stream)), "c21cm_field_moments_grids")
    return moments, hist


def bispectrum(field, shape, lengths, edges, triangles, *, offsets=(0,), row_pitch=None, stream=None):
    """Bispectra of ``len(offsets)`` boxes of ``shape`` = (nx, ny, nz) cells and ``lengths`` (Lx, Ly, Lz) read from
    the float32 array ``field`` (the layout of ``power_spectrum``: box b at flat element ``offsets[b] + (i ny + j)
    row_pitch + l``).  ``edges``: the n_bins + 1 shell edges in |k|; ``triangles``: (n, 3) shell indices b1 <= b2 <=
    b3.  Returns ``(bispectrum, n_triangles)``: float64 (n_batch, n) and int64 (n,), the closed mode triplets of
    each triangle (the same for every box); numpy for numpy input, torch on the field's device for a torch CUDA
    field.  The estimator is written down at ``c21cm_bispectrum_grids`` (include/c21cm_grid.h)."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    edges = np.ascontiguousarray(edges, np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("edges must be a 1-D array of at least 2 values")
    tri = np.asarray(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] < 1 or tri.dtype.kind not in "iu":
        raise ValueError("triangles must be an (n, 3) array of integers, n >= 1")
    tri = np.ascontiguousarray(tri, np.int32)
    n_tri = len(tri)
    if _is_torch(field):
        import torch

        out = torch.empty((n_batch, n_tri), dtype=torch.float64, device=field.device)
        counts = torch.empty((n_tri,), dtype=torch.int64, device=field.device)
    else:
        out, counts = np.empty((n_batch, n_tri)), np.empty((n_tri,), np.int64)
    bins = S.BispecBins(n_bins=len(edges) - 1, edges=edges.ctypes.data_as(S.c_double_p), n_triangles=n_tri,
                        triangles=tri.ctypes.data_as(C.POINTER(C.c_int)))
    Lx, Ly, Lz = (float(x) for x in lengths)
    lib = load()
    check(lib.c21cm_bispectrum_grids(_vptr(field), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p),
                                     Lx, Ly, Lz, C.byref(bins), _vptr(out), _vptr(counts), _stream(stream)),
          "c21cm_bispectrum_grids")
    return out, counts


def bubble_sizes(field, shape, lengths, edges, *, threshold=0.5, select_below=True, n_rays=1_000_000, seed=0,
                 los=False, periodic=(True, True, True), max_length=None, offsets=(0,), row_pitch=None,
                 return_rays=False, stream=None):
    """Mean-free-path bubble sizes of ``len(offsets)`` boxes of ``shape`` = (nx, ny, nz) cells and ``lengths`` (Lx,
    Ly, Lz) read from the float32 array ``field`` (the layout of ``power_spectrum``).  ``n_rays`` rays per box start
    in cells with ``v < threshold`` (``select_below``) or ``v >= threshold`` and run, isotropically or (``los``)
    along +-z, to the first cell that is not selected; ``edges``: the n_bins + 1 histogram edges in length.  Returns
    ``(hist, stats)``, int64 (n_batch, n_bins) and (n_batch, 4) = n_selected, n_ended, n_capped, n_escaped, and with
    ``return_rays`` also ``(lengths, flags, starts)``: float64, uint8 and int64 (n_batch, n_rays).  numpy for numpy
    input, torch on the field's device for a torch CUDA field.  The estimator is written down at
    ``c21cm_bubble_sizes_grids`` (include/c21cm_grid.h)."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    edges = np.ascontiguousarray(edges, np.float64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("edges must be a 1-D array of at least 2 values")
    n_bins = len(edges) - 1
    n_rays = int(n_rays)
    if not 1 <= n_rays <= 2**31 - 1:
        raise ValueError("n_rays must be in [1, 2^31 - 1]")
    seed = int(seed)
    if not 0 <= seed < 2**64:
        raise ValueError("seed must be in [0, 2^64)")
    Lx, Ly, Lz = (float(x) for x in lengths)
    max_length = max(Lx, Ly, Lz) if max_length is None else float(max_length)
    px, py, pz = (bool(p) for p in periodic)
    lengths_out = flags = starts = None
    if _is_torch(field):
        import torch

        def empty(shape_, dtype):
            return torch.empty(shape_, dtype=getattr(torch, dtype), device=field.device)
    else:
        def empty(shape_, dtype):
            return np.empty(shape_, dtype)
    hist, stats = empty((n_batch, n_bins), "int64"), empty((n_batch, 4), "int64")
    if return_rays:
        lengths_out, flags = empty((n_batch, n_rays), "float64"), empty((n_batch, n_rays), "uint8")
        starts = empty((n_batch, n_rays), "int64")
    lib = load()
    check(lib.c21cm_bubble_sizes_grids(
        _vptr(field), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p), Lx, Ly, Lz,
        float(threshold), int(bool(select_below)), n_rays, seed, int(bool(los)), px | (py << 1) | (pz << 2),
        max_length, n_bins, edges.ctypes.data_as(C.c_void_p), _vptr(hist), _vptr(stats), _vptr(lengths_out),
        _vptr(flags), _vptr(starts), _stream(stream)), "c21cm_bubble_sizes_grids")
    if return_rays:
        return hist, stats, lengths_out, flags, starts
    return hist, stats


def bubble_clusters(field, shape, edges, *, threshold=0.5, select_below=True, connectivity=1,
                    periodic=(True, True, True), offsets=(0,), row_pitch=None, return_labels=False, max_clusters=0,
                    stream=None):
    """Friends-of-friends clusters of the selected cells of ``len(offsets)`` boxes of ``shape`` = (nx, ny, nz) cells
    read from the float32 array ``field`` (the layout of ``power_spectrum``).  Cells with ``v < threshold``
    (``select_below``) or ``v >= threshold`` are joined to their neighbours: ``connectivity`` 1, 2, 3 = faces, and
    edges, and corners (6, 18, 26 neighbours), wrapping on the ``periodic`` axes.  ``edges``: the n_bins + 1 integer
    histogram edges in cells, the first >= 1.  Returns ``(hist_n, hist_cells, stats)``: int64 (n_batch, n_bins) the
    clusters per size bin and their cells, and (n_batch, 4) = n_selected, n_clusters, the cells of the largest cluster,
    its root (the smallest flat index of a cluster's cells; -1 without a selected cell); with ``return_labels`` also
    ``labels`` int32 (n_batch, nx ny nz), the root of every cell's cluster or -1; with ``max_clusters`` > 0 also
    ``(roots, sizes)`` int64 (n_batch, max_clusters), the first clusters in ascending root, padded with -1 / 0
    (``stats`` keeps the true count).  numpy for numpy input, torch on the field's device for a torch CUDA field.
    The estimator is written down at ``c21cm_bubble_clusters_grids`` (include/c21cm_grid.h)."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    if nx * ny * nz >= 2**31:
        raise ValueError("a box must have fewer than 2^31 cells")
    edges = np.ascontiguousarray(edges, np.int64)
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError("edges must be a 1-D array of at least 2 values")
    n_bins = len(edges) - 1
    connectivity = int(connectivity)
    if connectivity not in (1, 2, 3):
        raise ValueError("connectivity must be 1, 2 or 3")
    max_clusters = int(max_clusters)
    if max_clusters < 0:
        raise ValueError("max_clusters must be >= 0")
    px, py, pz = (bool(p) for p in periodic)
    labels = roots = sizes = None
    if _is_torch(field):
        import torch

        def empty(shape_, dtype):
            return torch.empty(shape_, dtype=getattr(torch, dtype), device=field.device)
    else:
        def empty(shape_, dtype):
            return np.empty(shape_, dtype)
    hist_n, hist_cells = empty((n_batch, n_bins), "int64"), empty((n_batch, n_bins), "int64")
    stats = empty((n_batch, 4), "int64")
    if return_labels:
        labels = empty((n_batch, nx * ny * nz), "int32")
    if max_clusters:
        roots, sizes = empty((n_batch, max_clusters), "int64"), empty((n_batch, max_clusters), "int64")
    lib = load()
    check(lib.c21cm_bubble_clusters_grids(
        _vptr(field), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p), float(threshold),
        int(bool(select_below)), connectivity, px | (py << 1) | (pz << 2), n_bins, edges.ctypes.data_as(C.c_void_p),
        _vptr(hist_n), _vptr(hist_cells), _vptr(stats), _vptr(labels), max_clusters, _vptr(roots), _vptr(sizes),
        _stream(stream)), "c21cm_bubble_clusters_grids")
    out = (hist_n, hist_cells, stats)
    if return_labels:
        out += (labels,)
    if max_clusters:
        out += (roots, sizes)
    return out


MINKOWSKI_MAX_THRESHOLDS = 255  # C21HIP_MINKOWSKI_MAX_THRESHOLDS


def minkowski(field, shape, thresholds, *, select_below=True, periodic=(True, True, True), offsets=(0,),
              row_pitch=None, stream=None):
    """The element counts behind the Minkowski functionals of the excursion sets of ``len(offsets)`` boxes of ``shape``
    = (nx, ny, nz) cells read from the float32 array ``field`` (the layout of ``power_spectrum``), at every one of the
    increasing ``thresholds`` (1 to 255 of them) from one read of the field.  At threshold t the cells with ``v < t``
    (``select_below``) or ``v >= t`` are selected, and an element of the cubical complex of the box -- which wraps on
    the ``periodic`` axes -- counts where a selected cell contains it.  Returns int64 (n_batch, n_thresholds, 8) =
    n3 (cells), n2x, n2y, n2z (faces perpendicular to an axis), n1x, n1y, n1z (edges parallel to one), n0 (vertices):
    numpy for numpy input, torch on the field's device for a torch CUDA field.  The estimator is written down at
    ``c21cm_minkowski_grids`` (include/c21cm_grid.h)."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    if nx * ny * nz >= 2**31:
        raise ValueError("a box must have fewer than 2^31 cells")
    thresholds = np.ascontiguousarray(thresholds, np.float64)
    if thresholds.ndim != 1 or not 1 <= thresholds.size <= MINKOWSKI_MAX_THRESHOLDS:
        raise ValueError(f"thresholds must be a 1-D array of 1 to {MINKOWSKI_MAX_THRESHOLDS} values")
    if not np.all(np.isfinite(thresholds)) or np.any(np.diff(thresholds) <= 0):
        raise ValueError("thresholds must be finite and strictly increasing")
    px, py, pz = (bool(p) for p in periodic)
    if _is_torch(field):
        import torch

        counts = torch.empty((n_batch, thresholds.size, 8), dtype=torch.int64, device=field.device)
    else:
        counts = np.empty((n_batch, thresholds.size, 8), np.int64)
    lib = load()
    check(lib.c21cm_minkowski_grids(
        _vptr(field), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p), int(thresholds.size),
        thresholds.ctypes.data_as(C.c_void_p), int(bool(select_below)), px | (py << 1) | (pz << 2), _vptr(counts),
        _stream(stream)), "c21cm_minkowski_grids")
    return counts


GRANULOMETRY_MAX_RADII = 255  # C21HIP_GRAN_MAX_RADII
EDT_NONE = 2**30  # C21CM_EDT_NONE: D2 of a box without an unselected cell


def granulometry(field, shape, radii2, *, threshold=0.5, select_below=True, periodic=(True, True, True), offsets=(0,),
                 row_pitch=None, return_dist2=False, return_level=False, stream=None):
    """The squared Euclidean distance transform and the granulometry of the selected cells of ``len(offsets)`` boxes of
    ``shape`` = (nx, ny, nz) cells read from the float32 array ``field`` (the layout of ``power_spectrum``).  Cells
    with ``v < threshold`` (``select_below``) or ``v >= threshold`` are selected; D2 of a cell is its squared distance,
    in cells and with the minimum image on the ``periodic`` axes, to the nearest unselected cell of its box (0 at
    unselected cells, ``EDT_NONE`` = 2^30 in a box without one).  ``radii2``: 0 to 255 increasing integer squared radii
    s >= 0.  Returns ``(covered, eroded, stats)``: int64 (n_batch, n_radii) the cells inside an inscribed ball with
    D2 > s and the cells with D2 > s, and (n_batch, 4) = n_selected, the largest D2 of a selected cell (0 without
    one), the smallest flat index attaining it (-1), n_unselected; with ``return_dist2`` also ``dist2`` int32
    (n_batch, nx ny nz); with ``return_level`` also ``level`` int32 (n_batch, nx ny nz), the number of radii at which
    the cell is covered, -1 at unselected cells.  numpy for numpy input, torch on the field's device for a torch CUDA
    field.  The estimator is written down at ``c21cm_granulometry_grids`` (include/c21cm_grid.h)."""
    nx, ny, nz = (int(x) for x in shape)
    row_pitch = nz if row_pitch is None else int(row_pitch)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n_batch = len(offsets)
    _f32_dense(field, "field")
    size = int(np.prod(field.shape, dtype=np.int64))
    if n_batch < 1 or offsets.min() < 0 or offsets.max() + (nx * ny - 1) * row_pitch + nz > size:
        raise ValueError("the boxes do not lie inside the field")
    if nx * ny * nz >= 2**31:
        raise ValueError("a box must have fewer than 2^31 cells")
    if nx * nx + ny * ny + nz * nz >= EDT_NONE:
        raise ValueError("nx^2 + ny^2 + nz^2 must be below 2^30")
    raw = np.asarray(radii2)
    if raw.ndim != 1 or raw.size > GRANULOMETRY_MAX_RADII:
        raise ValueError(f"radii2 must be a 1-D array of at most {GRANULOMETRY_MAX_RADII} values")
    if raw.size and raw.dtype.kind not in "iu" and not (np.all(np.isfinite(raw)) and np.all(raw == np.round(raw))):
        raise ValueError("squared radii must be integers (cells^2)")
    radii2 = np.ascontiguousarray(raw, np.int64)
    if np.any(radii2 < 0) or np.any(np.diff(radii2) <= 0):
        raise ValueError("squared radii must be >= 0 and strictly increasing")
    n_radii = int(radii2.size)
    px, py, pz = (bool(p) for p in periodic)
    if _is_torch(field):
        import torch

        def empty(shape_, dtype):
            return torch.empty(shape_, dtype=getattr(torch, dtype), device=field.device)
    else:
        def empty(shape_, dtype):
            return np.empty(shape_, dtype)
    covered, eroded = empty((n_batch, n_radii), "int64"), empty((n_batch, n_radii), "int64")
    stats = empty((n_batch, 4), "int64")
    dist2 = empty((n_batch, nx * ny * nz), "int32") if return_dist2 else None
    level = empty((n_batch, nx * ny * nz), "int32") if return_level else None
    lib = load()
    check(lib.c21cm_granulometry_grids(
        _vptr(field), nx, ny, nz, n_batch, row_pitch, offsets.ctypes.data_as(C.c_void_p), float(threshold),
        int(bool(select_below)), px | (py << 1) | (pz << 2), n_radii,
        radii2.ctypes.data_as(C.c_void_p) if n_radii else None, _vptr(covered) if n_radii else None,
        _vptr(eroded) if n_radii else None, _vptr(stats), _vptr(dist2), _vptr(level), _stream(stream)),
        "c21cm_granulometry_grids")
    out = (covered, eroded, stats)
    if return_dist2:
        out += (dist2,)
    if return_level:
        out += (level,)
    return out


OBSERVE_MAX_SIGMA = 128.0  # C21HIP_OBSERVE_MAX_LW / 4


def observe_geometry():
    """``(tile_rows, lds_lw)`` of the beam kernel as the library was built: the cells of a transverse line, halo
    included, that a workgroup holds at a time, and the widest half kernel that goes through LDS."""
    rows, lw = C.c_int(0), C.c_int(0)
    load().c21hip_observe_geometry(C.byref(rows), C.byref(lw))
    return rows.value, lw.value


def observe_smooth(field, sigma_cells, los_below=None, los_above=None, *, periodic_los=False, subtract_mean=True,
                   out=None, stream=None):
    """Telescope-resolution smoothing of the float32 ``field`` (nx, ny, ns), the line of sight the last and fastest
    axis: the fp64 mean of every slice (subtracted with ``subtract_mean``), a Gaussian beam of ``sigma_cells[s]`` cells
    across the line of sight, truncated at 4 sigma and wrapping, and the mean over the slices ``s - los_below[s] ..
    s + los_above[s]`` along it, clipped to the line or, with ``periodic_los``, wrapped.  ``sigma_cells``: a scalar
    or ns values; the counts: ns integers each, all 0 where left out.  Returns ``(out, slice_means)``, float32
    shaped as the field and float64 (ns,): numpy for numpy input, torch on the field's device for a torch CUDA field,
    which never visits the host.  ``out``: an array of the field's kind to write into; it must not overlap the field.
    The definition is written down at ``c21cm_observe_smooth_grids`` (include/c21cm_grid.h)."""
    if field.ndim != 3:
        raise ValueError(f"field must be a 3-D (nx, ny, ns) array, got {field.ndim} dimensions")
    _f32_dense(field, "field")
    nx, ny, ns = (int(x) for x in field.shape)
    if min(nx, ny, ns) < 1:
        raise ValueError("every axis needs at least 1 cell")
    if nx * ny * ns >= 2**31:
        raise ValueError("a field must have fewer than 2^31 cells")
    sigma = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_cells, np.float64), (ns,)))

    def counts(a, what):
        if a is None:
            return np.zeros(ns, np.int32)
        a = np.asarray(a)
        if a.shape != (ns,) or a.dtype.kind not in "iu":
            raise ValueError(f"{what} must be {ns} integers")
        if np.any(a > 2**31 - 1) or np.any(a < -2**31):
            raise ValueError(f"{what} must fit 32 bits")
        return np.ascontiguousarray(a, np.int32)

    below, above = counts(los_below, "los_below"), counts(los_above, "los_above")
    if _is_torch(field):
        import torch

        if out is None:
            out = torch.empty_like(field)
        means = torch.empty(ns, dtype=torch.float64, device=field.device)
        same_kind = _is_torch(out) and out.device == field.device
    else:
        if out is None:
            out = np.empty_like(field)
        means = np.empty(ns, np.float64)
        same_kind = not _is_torch(out)
    if not same_kind or tuple(out.shape) != (nx, ny, ns):
        raise ValueError("out must be an array of the field's kind, device and shape")
    _f32_dense(out, "out")
    check(load().c21cm_observe_smooth_grids(
        _vptr(field), nx, ny, ns, sigma.ctypes.data_as(C.c_void_p), below.ctypes.data_as(C.c_void_p),
        above.ctypes.data_as(C.c_void_p), int(bool(periodic_los)), int(bool(subtract_mean)), _vptr(out), _vptr(means),
        _stream(stream)), "c21cm_observe_smooth_grids")
    return out, means
