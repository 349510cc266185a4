"""Thin Python harness over the C ABI of libamplisolve_hip.so.

torch is used only for plumbing: device memory (tensors), the current HIP
stream and torch.distributed.  Every number comes out of the HIP kernels; when
the library or the GPU is missing the calls raise AmpliError.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import inspect
from dataclasses import dataclass

from ._lib import (CONSTANTS, AccTable, AllelicParams, AmpliError, AmpliNoDevice, Call, DiluteMix, FractionParams, GenotypeParams, LooCall, MonitorParams, Records,
                   hip_lib)

# Every numeric AMPLI_X of the headers is this module's X, with the header's value (_lib.CONSTANTS).  Which family goes with what:
#   POISSON_FULL / _PREFILTER              the mode of poisson_call, poisson_call_records and loo_call
#   CALL_SHARDS, CALL_COUNTER_*            the compact call list (read_calls, read_loo_calls, n_calls_total)
#   RECORDS_*                              the record layouts (Context.LAYOUTS)
#   LIMIT_*                                detection_limits: status in bits 0-2, LIMIT_CALLED, LIMIT_RECHECK, the counters
#   DISPERSION_*                           panel_dispersion's status
#   GENO_PLANES, RELATION_*                genotype_planes, and the relation of ampli_host_concordance_relation
#   CONTAM_*                               the nine sums of contamination
#   AMP_*, AMPLICON_*, GENE_*              the four sums of amplicon_depth; amplicon_reference's statuses, the limit of N / A in the two
#                                          stage-2 calls and the rows a wave of the depth kernel owns; ampli_host_amplicon_gene_status
#   SPEC_*, SPECTRUM_*                     the nine sums of spectrum; its limit of C, the rows of a workgroup, the classes, types and
#                                          channels of the command line's folds and the statuses of ampli_host_spectrum_score
#   EXCEEDANCE_*                           exceedance: the cell that is not evaluated, the most normals of a panel, the launch shape
#   NB_NA, PAIR_NA, FDR_NA                 a cell of nb_score / pair_score that is not evaluated, of fdr_adjust that is not tested
#   DILUTE_BAD_*                           the flag word of a mixture of dilute
#   MON_*                                  the six sums of monitor_sums, the score without an evaluated entry, the verdicts, the strip
#   TF_*                                   tumour_fraction: the four values and two counts of a (sample, list), the value where nothing is
#                                          estimated, the bisection's steps, the z2 of three confidence levels, verdicts and changes
#   AI_*                                   allelic imbalance: the planes of the het-site reference, the status of a cell (code = status *
#                                          8 + pair, AI_NO_PAIR: none), the untested score, the five sums of a region and the verdicts
#   INDEL_LEN_BINS                         indel_count: the length bins per (position, kind) of its second output
#   EVIDENCE_*                             read_evidence: the metrics per (position, nt), their indices and the bins of each
#   PHASE_*                                phase.read_phase: the partners of a key, the states of a read at a key and the state OTHER
globals().update({name[len("AMPLI_"):]: value for name, value in CONSTANTS.items()})

# Python's own
NT = "ACGT"
GENO_V, GENO_A, GENO_C, GENO_G, GENO_T, GENO_H = (CONSTANTS["AMPLI_GENO_" + x].bit_length() - 1 for x in "VACGTH")  # planes: the headers hold the bits
CONC_SITES, CONC_MATCH, CONC_IBS0, CONC_HET_EITHER, CONC_HET_MATCH = range(5)  # the counts of Context.concordance
CONTAM_UNDETERMINED, CONTAM_CLEAN, CONTAM_CONTAMINATED = (CONSTANTS["AMPLI_CONTAM_STATUS_" + x] for x in ("UNDETERMINED", "CLEAN", "CONTAMINATED"))
DILUTE_KEEP_ALL = 1 << 32  # the threshold of dilute that keeps every read


def _ok(t, dtype, shape=None) -> bool:
    """Is t a contiguous device tensor of dtype and shape?  None in shape is an axis of any size, a leading ... any leading axes."""
    if not (t.dtype == dtype and t.is_cuda and t.is_contiguous()):
        return False
    if shape is None:
        return True
    have = tuple(t.shape)
    if shape and shape[0] is ...:
        shape = shape[1:]
        have = have[len(have) - len(shape):]
    return len(have) == len(shape) and all(want is None or want == got for want, got in zip(shape, have))


def _fields(struct):
    """the members of a ctypes struct as a flat numpy field list, a nested struct's in its place"""
    import numpy as np

    out = []
    for name, t in struct._fields_:
        out += _fields(t) if issubclass(t, C.Structure) else [(name, np.dtype(t))]
    return out


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _on_stream(fn):
    """fn(self, ...) with the context's stream as torch's current stream (the contract in Context's docstring): every torch allocation,
    fill, upload and readback inside fn is then ordered on it and comes from its pool of the caching allocator.  Where the context's
    stream is already current -- the default context -- fn runs as it is: one look at torch's current stream per call."""
    @functools.wraps(fn)
    def on_stream(self, *args, **kw):
        import torch

        if self.stream is None or torch.cuda.current_stream(self.device).cuda_stream == self._stream_ptr:
            return fn(self, *args, **kw)
        with torch.cuda.stream(self.stream):
            return fn(self, *args, **kw)

    on_stream.on_stream = True
    return on_stream


class _StaticOrBound:
    """fn(ctx_or_None, ...) as a method that may also be called on the class, as the static method it once was: ctx is then None"""

    def __init__(self, fn):
        self.fn = fn
        functools.update_wrapper(self, fn)

    def __get__(self, obj, cls=None):
        return functools.partial(self.fn, obj)


class Acc:
    """Accumulator table (ampli_acc_table) living in one device buffer."""

    def __init__(self, ctx: "Context | None", P: int, buf=None, device=None):
        """ctx may be None for a host-side table (layout functions need no GPU): pass device="cpu"."""
        import torch

        lib = ctx.lib if ctx is not None else hip_lib()
        self.P = int(P)
        nbytes = lib.ampli_acc_bytes(self.P)
        dev = device if device is not None else ctx.device
        if buf is None:
            # over-allocate on the host so the base can be 256-byte aligned like a device allocation; a device table comes from the pool
            # of the context's stream
            with (torch.cuda.stream(ctx.stream) if ctx is not None and device is None and ctx.stream is not None else contextlib.nullcontext()):
                raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
            off = (-raw.data_ptr()) % 256
            buf = raw[off: off + nbytes]
        self.buf = buf
        assert self.buf.numel() >= nbytes and self.buf.data_ptr() % 256 == 0
        self.struct = AccTable()
        rc = lib.ampli_acc_bind(_ptr(self.buf), self.P, C.byref(self.struct))
        if rc != 0:
            raise AmpliError("ampli_acc_bind failed")
        base = self.buf.data_ptr()

        def view(ptr, dtype, shape):
            n = 1
            for d in shape:
                n *= d
            off = ptr - base
            return self.buf[off: off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(*shape)

        s = self.struct
        P_ = self.P
        self.snt = view(s.snt, torch.float64, (2, 4, P_))
        self.srd = view(s.srd, torch.int64, (2, 4, P_))
        self.cnt = view(s.cnt, torch.int32, (4, P_))
        self.nrec = view(s.nrec, torch.int32, (P_,))
        self.gm_n = view(s.gm_n, torch.int32, (4, P_))
        self.gm_first = view(s.gm_first, torch.int32, (4, P_))
        self.gm_first_af = view(s.gm_first_af, torch.float32, (4, P_))
        self.gm_rest = view(s.gm_rest, torch.float32, (4, P_))

    def planes(self):
        return dict(snt=self.snt, srd=self.srd, cnt=self.cnt, nrec=self.nrec, gm_n=self.gm_n,
                    gm_first=self.gm_first, gm_first_af=self.gm_first_af, gm_rest=self.gm_rest)


@dataclass
class ErrorTable:
    rate: "object"          # [2,4,P] float32
    code: "object"          # [4,P] uint8
    thr: "object"           # [2,4,P] float32 (after the text round trip)
    germ_val: "object"      # [4,P] float32
    germ_present: "object"  # [4,P] uint8
    flags: "object"         # [1] int32


class Context:
    """One device, one stream, and every entry point of libamplisolve_hip.so as a method.

    The stream contract.  The context's stream is torch's current stream at the time the context is created
    (`with torch.cuda.stream(s): ctx = Context(0)`); Context.stream is that torch.cuda.Stream.
      * Every device operation a method causes is ordered on the context's stream, whatever torch's current stream is when the method
        is called: the kernels, the fills of outputs that are added to, the uploads of host arrays and the readbacks.
      * Tensors a method returns are valid in that stream's order (and come from that stream's pool of torch's caching allocator): use
        them under torch.cuda.stream(ctx.stream), or after ctx.sync(), or make the other stream wait on an event of this one.
      * A method that returns host values (flags, pack16 / pack24's fits, read_calls, read_loo_calls, n_calls_total, the limit and power
        statistics) synchronises that stream and no other.  acc_merge synchronises it too (include/amplisolve_hip.h).
    Tensors the caller brings are read and written in the same order: what fills them has to be ordered before the call on the
    context's stream.  The setters, getters, event and graph handles cause no device operation of torch's and are not wrapped.
    With own_stream=True the kernels run on a stream of the library's own (hipStreamNonBlocking) and Context.stream is None: torch's
    part of a method -- allocations, fills, uploads, readbacks -- stays on torch's current stream, and ordering the two is the
    caller's business (bring every output, or ctx.sync() and torch.cuda.synchronize() between the steps), as before."""

    def __init__(self, device: int = 0, own_stream: bool = False):
        import torch

        self.lib = hip_lib()
        # two different probes, two different messages (a failure here once could not be told apart afterwards)
        msg = C.create_string_buffer(256)
        n = self.lib.ampli_device_probe(msg, len(msg))
        if n <= 0:
            why = msg.value.decode() if n < 0 else "hipGetDeviceCount succeeded and counted 0 devices"
            raise AmpliNoDevice(f"no MI355X visible to libamplisolve_hip.so ({why}); there is no CPU fallback")
        if not torch.cuda.is_available():
            raise AmpliError(f"libamplisolve_hip.so sees {n} device(s) but torch.cuda.is_available() is False "
                             f"(torch {torch.__version__}, hip {getattr(torch.version, 'hip', None)}): the tensors this API hands out need torch's runtime")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        stream = C.c_void_p(-1) if own_stream else C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        h = C.c_void_p()
        rc = self.lib.ampli_ctx_create(device, stream, C.byref(h))
        if rc != 0:
            raise AmpliError(f"ampli_ctx_create: {self.lib.ampli_strerror(rc).decode()}")
        self.h = h
        self.own_stream = own_stream
        # the context's stream as torch knows it: the caller's torch.cuda.Stream.  A context that owns its stream (own_stream=True) has
        # none: its methods' torch operations stay on torch's current stream, as they always were ("left out")
        self._stream_ptr = int(self.lib.ampli_stream(self.h) or 0)
        self.stream = None if own_stream else torch.cuda.current_stream(self.device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ampli_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            detail = self.lib.ampli_last_error(self.h).decode() if getattr(self, "h", None) else ""
            raise AmpliError(f"{self.lib.ampli_strerror(rc).decode()} ({rc}): {detail}")

    def sync(self):
        self._check(self.lib.ampli_sync(self.h))

    # ---- what the methods below share -------------------------------------------------------
    def _out(self, t, dtype, shape, zero: bool = False):
        """the caller's buffer or a new one (zeroed where the kernel adds to it), checked either way"""
        import torch

        if t is None:
            t = (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=self.device)
        assert _ok(t, dtype, shape)
        return t

    def _levels(self, levels):
        """allele-fraction levels as float32 on the device, or None without any.  Uploaded once per distinct set: an upload from pageable
        host memory waits for everything enqueued on the stream, which would make detection_limits / detection_power synchronous."""
        import torch

        key = tuple(float(x) for x in levels)
        if not key:
            return None
        cache = self.__dict__.setdefault("_level_sets", {})
        if key not in cache:
            if len(cache) >= 64:
                cache.clear()
            cache[key] = torch.tensor(key, dtype=torch.float32, device=self.device)
        return cache[key]

    def _csr(self, off, ent, max_len: int, bound: int):
        """Position lists as a CSR on the device: (off int32 [n + 1], ent int32 [W] -- both read as uint32 --, W).  Host arrays are
        checked (monotone offsets, fewer than max_len entries, each in [0, bound)) and uploaded; device tensors are taken as they are."""
        import numpy as np
        import torch

        if not isinstance(off, torch.Tensor):
            o, e = np.asarray(off, np.int64), np.asarray(ent, np.int64)
            assert o.ndim == 1 and len(o) >= 2 and o[0] >= 0 and (np.diff(o) >= 0).all() and o[-1] <= len(e) < max_len
            assert ((e >= 0) & (e < bound)).all()
            off = torch.from_numpy(o.astype(np.uint32).view(np.int32)).to(self.device)
            ent = torch.from_numpy((e if len(e) else np.zeros(1, np.int64)).astype(np.uint32).view(np.int32)).to(self.device)
            W = len(e)
        else:
            W = ent.numel()
            if W == 0:  # a pointer is required even where nothing is read through it
                ent = torch.zeros((1,), dtype=torch.int32, device=self.device)
        assert _ok(off, torch.int32, (None,)) and _ok(ent, torch.int32, (None,))
        return off, ent, W

    def _positions_u8(self, x, P: int):
        """uint8 [P] on the device (ref_code, a class per position): a device tensor, or a host array, which is checked and uploaded"""
        import numpy as np
        import torch

        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            assert x.dtype == np.uint8 and x.shape == (P,)
            x = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        assert _ok(x, torch.uint8, (P,))
        return x

    def _call_list(self, rows: int, R: int, entry, capacity: int, call_mask, calls_buf, n_calls):
        """What the caller did not bring of a compact call list: the mask [rows, R] in a buffer of whole 4-byte words, room for
        `capacity` entries, the shard counters.  Returns them with the capacity cut to whole shards."""
        import torch

        d = self.device
        if call_mask is None:
            call_mask = torch.empty(((rows * R + 3) // 4 * 4,), dtype=torch.uint8, device=d)[: rows * R].view(rows, R)
        if capacity > 0 and calls_buf is None:
            calls_buf = torch.empty((capacity * C.sizeof(entry),), dtype=torch.uint8, device=d)
        if capacity > 0:
            capacity -= capacity % CALL_SHARDS
        if capacity > 0 and n_calls is None:
            n_calls = torch.zeros((CALL_COUNTER_WORDS,), dtype=torch.int64, device=d)
        return call_mask, calls_buf, capacity, n_calls

    def _read_list(self, res, entry):
        """the compact list of `entry` structs on the host, sorted by (sample, record, alt): a numpy record array of the struct's members"""
        import numpy as np

        counts = res["n_calls"][::CALL_COUNTER_STRIDE].cpu().numpy()
        per = res["capacity"] // CALL_SHARDS
        if (counts > per).any():
            raise AmpliError(f"call list segment overflowed: {int(counts.max())} > {per}; rerun with a larger capacity")
        sz = C.sizeof(entry)
        raw = b"".join(res["calls_buf"][k * per * sz: (k * per + int(counts[k])) * sz].cpu().numpy().tobytes() for k in range(CALL_SHARDS))
        dt = np.dtype(_fields(entry))
        assert dt.itemsize == sz
        a = np.frombuffer(raw, dtype=dt)
        return a[np.lexsort((a["alt"], a["record"], a["sample"]))]

    # ---- record layout (include/amplisolve_hip.h: AMPLI_RECORDS_*) ----
    LAYOUTS = {"i32": RECORDS_I32, "u16": RECORDS_U16, "u24": RECORDS_U24}

    def _rec_dtype(self):
        import torch

        return {"i32": torch.int32, "u16": torch.int16, "u24": torch.uint8}[getattr(self, "_layout", "i32")]

    def _rec_elems(self) -> int:
        """elements of _rec_dtype per record"""
        return 24 if getattr(self, "_layout", "i32") == "u24" else 8

    def set_record_layout(self, layout):
        """Every record tensor handed to this context from now on is int32 [S, R, 8] ("i32"), int16 [S, R, 8] ("u16")
        or uint8 [S, R, 24] ("u24": 8 little-endian 24-bit fields).  True / False select "u16" / "i32"."""
        if isinstance(layout, bool):
            layout = "u16" if layout else "i32"
        self._check(self.lib.ampli_set_record_layout(self.h, self.LAYOUTS[layout]))
        self._layout = layout

    def pack16(self, recs):
        """int32 [S, R, 8] records -> (int16 [S, R, 8] records, fits): fits is False when a count exceeds 65534."""
        import torch

        assert _ok(recs, torch.int32, (..., 8))
        out = torch.empty(recs.shape, dtype=torch.int16, device=recs.device)
        over = torch.zeros((1,), dtype=torch.int32, device=recs.device)
        self._check(self.lib.ampli_records_pack16(self.h, _ptr(recs), recs.numel() // 8, _ptr(out), _ptr(over)))
        return out, int(over.item()) == 0

    def pack24(self, recs):
        """int32 [S, R, 8] records -> (uint8 [S, R, 24] records, fits): fits is False when a count exceeds 2^24 - 2."""
        import torch

        assert _ok(recs, torch.int32, (..., 8))
        out = torch.empty(tuple(recs.shape[:-1]) + (24,), dtype=torch.uint8, device=recs.device)
        over = torch.zeros((1,), dtype=torch.int32, device=recs.device)
        self._check(self.lib.ampli_records_pack24(self.h, _ptr(recs), recs.numel() // 8, _ptr(out), _ptr(over)))
        return out, int(over.item()) == 0

    def pack(self, recs, layout: str):
        """recs (int32) in `layout`: (tensor, fits)"""
        return (recs, True) if layout == "i32" else (self.pack16(recs) if layout == "u16" else self.pack24(recs))

    def set_tuning(self, reduce_splits: int = 0, general: bool = False, groups: int = 0):
        self._check(self.lib.ampli_set_tuning(self.h, reduce_splits, int(general), groups))

    def last_reduce_kernel(self) -> str:
        """the kernel the latest error_reduce launch of this context was"""
        k = self.lib.ampli_last_reduce_kernel(self.h)
        self._check(min(k, 0))
        return {1: "error_reduce_u16_kernel", 2: "error_reduce_u24_kernel"}.get(k, "error_reduce_kernel")

    # ---- hipGraph capture ---------------------------------------------------------------
    def graph_begin(self):
        self._check(self.lib.ampli_graph_begin(self.h))

    def graph_end(self):
        g = C.c_void_p()
        self._check(self.lib.ampli_graph_end(self.h, C.byref(g)))
        return g

    def graph_launch(self, g):
        self._check(self.lib.ampli_graph_launch(self.h, g))

    def graph_destroy(self, g):
        self.lib.ampli_graph_destroy(g)

    def set_async_drain(self, on: bool):
        """poisson_call's drain kernel on a side stream; results complete after wait_calls() / sync()."""
        self._check(self.lib.ampli_set_async_drain(self.h, int(on)))

    def wait_calls(self):
        self._check(self.lib.ampli_wait_calls(self.h))

    def set_ranges(self, n: int):
        """error_estimate / poisson_call (prefilter) over n tile-aligned position ranges on n streams (include/amplisolve_hip.h,
        ampli_set_ranges); 1 = off.  The section closes at the next other call on this context."""
        self._check(self.lib.ampli_set_ranges(self.h, n))

    def ranges_concurrent(self) -> bool:
        """did ampli_set_ranges see every pair of the ranges' streams overlap (different hardware queues)?"""
        return self.lib.ampli_ranges_concurrent(self.h) == 1

    def ranges_join(self):
        self._check(self.lib.ampli_ranges_join(self.h))

    def range_record(self, rng: int, ev):
        """record `ev` on range `rng`'s stream without closing the section (ampli_range_event_record)"""
        self._check(self.lib.ampli_range_event_record(self.h, rng, ev))

    def set_reduce_compact(self, on):
        """True / False; 2 = the compact-state kernel for uint16 records only (A/B runs of its 24-bit form)"""
        self._check(self.lib.ampli_set_reduce_compact(self.h, 2 if on == 2 else int(bool(on))))

    def set_slice_format(self, slim: bool):
        """sums of the sliced exchange as 14 packed planes (slim) or 21 plain ones (ampli_set_slice_format)"""
        self._check(self.lib.ampli_set_slice_format(self.h, 1 if slim else 0))

    def set_poisson_tuning(self, rows_per_wave: int = 0, drain_blocks: int = 0):
        """poisson_call launch shape (ampli_set_poisson_tuning); 0 = default.  Results do not depend on it."""
        self._check(self.lib.ampli_set_poisson_tuning(self.h, rows_per_wave, drain_blocks))

    def set_queue_items(self, items: int):
        self._check(self.lib.ampli_set_queue_items(self.h, items))

    def flags(self, clear: bool = True) -> int:
        """AMPLI_FLAG_* raised by kernels since the last clear (synchronises)."""
        out = C.c_int32()
        self._check(self.lib.ampli_ctx_flags(self.h, C.byref(out), int(clear)))
        return int(out.value)

    # ---- events on the context's stream -------------------------------------------------
    def event(self):
        ev = C.c_void_p()
        self._check(self.lib.ampli_event_create(C.byref(ev)))
        return ev

    def record(self, ev):
        self._check(self.lib.ampli_event_record(self.h, ev))

    def elapsed_ms(self, a, b) -> float:
        ms = C.c_float()
        self._check(self.lib.ampli_event_elapsed_ms(a, b, C.byref(ms)))
        return float(ms.value)

    # ---- kernels ---------------------------------------------------------------------
    def new_acc(self, P: int) -> Acc:
        return Acc(self, P)

    def error_reduce(self, recs, P: int, C_value: float = 0.002, cov: int = 100, E: int = 0, dup_off=None,
                     first_sample: int = 0, acc: Acc | None = None) -> Acc:
        assert _ok(recs, self._rec_dtype())
        S = recs.shape[0]
        assert recs.numel() == S * (P + E) * self._rec_elems()
        if acc is None:
            acc = self.new_acc(P)
        self._check(self.lib.ampli_error_reduce(self.h, _ptr(recs), P, E, _ptr(dup_off), S, first_sample,
                                                C_value, cov, C.byref(acc.struct)))
        return acc

    def records(self, recs, layout: str, n_samples: int, E: int = 0, row_stride: int = 0, ext=None, ext_stride: int = 0,
                dup_off=None, ext_pos=None, rd=None, rd_ext=None) -> Records:
        """ampli_records over device tensors (the caller keeps them alive).  rd / rd_ext: int32 [n][P] / [n][E] RD column of
        lines whose RD is not A+C+G+T (INT32_MIN elsewhere)."""
        r = Records(recs.data_ptr(), row_stride, ext.data_ptr() if ext is not None else None, ext_stride, E,
                    dup_off.data_ptr() if dup_off is not None else None, ext_pos.data_ptr() if ext_pos is not None else None,
                    self.LAYOUTS[layout], n_samples, rd.data_ptr() if rd is not None else None,
                    rd_ext.data_ptr() if rd_ext is not None else None)
        r._keep = (recs, ext, dup_off, ext_pos, rd, rd_ext)
        return r

    def error_reduce_records(self, rec: Records, P: int, acc: Acc | None, C_value: float = 0.002, cov: int = 100, first_sample: int = 0,
                             accumulate: bool = False, out: ErrorTable | None = None, finalize: bool = False, summary: bool = False):
        """One chunk of a cohort into `acc` (accumulate: acc (+) chunk); finalize: also the error table of the merged state.
        summary: `acc` is streaming state only (AMPLI_REDUCE_SUMMARY: gm_n may saturate at two, gm_first may read -1), which lets
        the compact-state kernel carry it."""
        if finalize and out is None:
            out = self._new_error_table(P)
        o = out if finalize else None
        self._check(self.lib.ampli_error_reduce_records(self.h, C.byref(rec), P, first_sample, C_value, cov,
                                                        C.byref(acc.struct) if acc is not None else None, int(bool(accumulate)) | (2 if summary else 0),
                                                        _ptr(o.rate) if o else None, _ptr(o.code) if o else None, _ptr(o.thr) if o else None,
                                                        _ptr(o.germ_val) if o else None, _ptr(o.germ_present) if o else None,
                                                        _ptr(o.flags) if o else None))
        return out

    def error_sums_inorder(self, rec: Records, P: int, acc: Acc, C_value: float = 0.002, cov: int = 100, accumulate: bool = False):
        """acc.snt in the reference's own order of addition (ampli_error_sums_inorder): one chunk, last sample first; a cohort in several
        chunks from its LAST chunk (accumulate=False) to its first (True).  The other planes of acc are left alone."""
        self._check(self.lib.ampli_error_sums_inorder(self.h, C.byref(rec), P, C_value, cov, C.byref(acc.struct), int(bool(accumulate))))

    def error_reduce_records_sliced(self, rec: Records, P: int, acc: Acc | None, n_slices: int, sums, gm, C_value: float = 0.002, cov: int = 100,
                                    first_sample: int = 0, accumulate: bool = False, summary: bool = True):
        """The last chunk of a shard's streamed cohort: acc (+) chunk straight into the slice-major exchange buffers."""
        self._check(self.lib.ampli_error_reduce_records_sliced(self.h, C.byref(rec), P, first_sample, C_value, cov,
                                                               C.byref(acc.struct) if acc is not None else None,
                                                               int(bool(accumulate)) | (2 if summary else 0), n_slices, _ptr(sums), _ptr(gm)))

    def poisson_call_records(self, rec: Records, P: int, thr, ref_code, cov: int = 100, mode: int = POISSON_PREFILTER,
                             call_mask=None, capacity: int = 0, calls_buf=None, n_calls=None, q=None, af=None):
        """q / af: the caller's buffers for the dense scores (float64 [T, R, 4, 2], all-scores mode only) and VAFs (float32 [T, R, 4, 3])"""
        call_mask, calls_buf, capacity, n_calls = self._call_list(rec.n_samples, P + rec.E, Call, capacity, call_mask, calls_buf, n_calls)
        self._check(self.lib.ampli_poisson_call_records(self.h, C.byref(rec), P, _ptr(thr), _ptr(ref_code), cov, mode, _ptr(call_mask),
                                                        _ptr(calls_buf), capacity, _ptr(n_calls), _ptr(q), _ptr(af)))
        return dict(call_mask=call_mask, q=q, af=af, calls_buf=calls_buf, n_calls=n_calls, capacity=capacity)

    def detection_limits(self, rec: Records, P: int, thr, ref_code, cov: int = 100, levels=(), counts=None):
        """Detection limits of the calling gate for one resident chunk (ampli_limit_records): per record and base the smallest
        alternative counts (forward, reverse) with which the gate would pass on that line's own depths.  Returns min_reads int32
        [n, P + E, 4, 2], status uint8 [n, P + E, 4] (LIMIT_* in bits 0-2, LIMIT_CALLED, LIMIT_RECHECK: to be settled with
        ampli_host_limit_reads) and counts int64 [n, 6 + len(levels)] (added to when given): lines without a reference base, pairs OK /
        LOWDEPTH / NOESTIMATE / UNREACHABLE / RECHECK, and per level the OK pairs with MinAF <= level."""
        import torch

        n, R = rec.n_samples, P + rec.E
        d = self.device
        lv = self._levels(levels)
        min_reads = torch.empty((n, R, 4, 2), dtype=torch.int32, device=d)
        status = torch.empty((n, R, 4), dtype=torch.uint8, device=d)
        if counts is None:
            counts = torch.zeros((n, LIMIT_COUNTERS + len(levels)), dtype=torch.int64, device=d)
        self._check(self.lib.ampli_limit_records(self.h, C.byref(rec), P, _ptr(thr), _ptr(ref_code), cov, _ptr(lv), len(levels), _ptr(min_reads),
                                                 _ptr(status), _ptr(counts)))
        return dict(min_reads=min_reads, status=status, counts=counts)

    def limit_stats(self, reset: bool = False):
        """(strands searched, scorer evaluations, the most evaluations of one strand) of this context's detection_limits calls"""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.ampli_limit_stats(self.h, out, int(reset)))
        return int(out[0]), int(out[1]), int(out[2])

    def detection_power(self, rec: Records, P: int, min_reads, status, levels=(), confidence: float = 0.95, counts=None, want_power: bool = True,
                        want_lod: bool = True):
        """Detection power and limit of detection for one resident chunk (ampli_power_records).  min_reads / status as detection_limits
        returns them, the RECHECK cells settled.  Returns power float32 [n, P + E, 4, len(levels)] (the probability that a variant at
        that allele fraction passes the gate; None with want_power=False), lod float32 [n, P + E, 4] (the allele fraction called with
        probability `confidence`, in [0.5, 0.99]; None with want_lod=False) -- both 0 in every cell that is not OK -- and counts int64
        [n, 1 + len(levels)] (added to when given): OK pairs, and per level the OK pairs with power >= confidence."""
        import torch

        n, R = rec.n_samples, P + rec.E
        d = self.device
        lv = self._levels(levels)
        power = torch.empty((n, R, 4, len(levels)), dtype=torch.float32, device=d) if want_power else None
        lod = torch.empty((n, R, 4), dtype=torch.float32, device=d) if want_lod else None
        if counts is None:
            counts = torch.zeros((n, 1 + len(levels)), dtype=torch.int64, device=d)
        self._check(self.lib.ampli_power_records(self.h, C.byref(rec), P, _ptr(min_reads), _ptr(status), _ptr(lv), len(levels), confidence,
                                                 _ptr(power), _ptr(lod), _ptr(counts)))
        return dict(power=power, lod=lod, counts=counts)

    def power_stats(self, reset: bool = False):
        """(tails evaluated, pmf terms summed, the most terms of one tail) of this context's detection_power calls"""
        out = (C.c_uint64 * 3)()
        self._check(self.lib.ampli_power_stats(self.h, out, int(reset)))
        return int(out[0]), int(out[1]), int(out[2])

    def dispersion_records(self, rec: Records, P: int, acc0: Acc, cov: int, x2, rinv, accumulate: bool = False, sample_x2=None,
                           sample_expect=None, sample_terms=None):
        """One resident chunk into the dispersion planes (ampli_dispersion_records): x2 / rinv float64 [2, 4, P] are overwritten or,
        with accumulate, added to; the three sample arrays (float64, float64, int64 [n]) are overwritten, or all None."""
        self._check(self.lib.ampli_dispersion_records(self.h, C.byref(rec), P, C.byref(acc0.struct), cov, _ptr(x2), _ptr(rinv), int(bool(accumulate)),
                                                      _ptr(sample_x2), _ptr(sample_expect), _ptr(sample_terms)))

    def dispersion_finalize(self, P: int, acc0: Acc, x2, rinv, z_cutoff: float, z, phi, status, counts):
        """z (float64), phi (float32) and status (uint8), each [2, 4, P], from the summed planes (ampli_dispersion_finalize); counts int64
        [4] is added to."""
        self._check(self.lib.ampli_dispersion_finalize(self.h, P, C.byref(acc0.struct), _ptr(x2), _ptr(rinv), float(z_cutoff), _ptr(z), _ptr(phi),
                                                       _ptr(status), _ptr(counts)))

    def panel_dispersion(self, chunks, P: int, acc0: Acc, cov: int = 100, z_cutoff: float = 4.0, samples: bool = True):
        """Per-position dispersion of a panel of normals and per-normal outlier scores.  chunks: the Records of the resident
        cohort in visit order; acc0: the WHOLE cohort's table reduced with C_value = 0 and the same cov (error_reduce_records over every
        chunk, summary=True is enough).  Returns x2, rinv, z (float64), phi (float32), status (uint8: DISPERSION_OK / _FEW in bits 0-2,
        DISPERSION_HIGH where z >= z_cutoff), each [2, 4, P]; counts int64 [4] (cells OK, FEW, HIGH, positions with a HIGH cell); and,
        with samples, sample_x2, sample_expect (float64) and sample_terms (int64) over all normals in visit order."""
        import torch

        d = self.device
        x2 = torch.empty((2, 4, P), dtype=torch.float64, device=d)
        rinv = torch.empty((2, 4, P), dtype=torch.float64, device=d)
        S = sum(r.n_samples for r in chunks)
        sx = torch.empty((S,), dtype=torch.float64, device=d) if samples else None
        se = torch.empty((S,), dtype=torch.float64, device=d) if samples else None
        stm = torch.empty((S,), dtype=torch.int64, device=d) if samples else None
        lo = 0
        for i, rec in enumerate(chunks):
            hi = lo + rec.n_samples
            self.dispersion_records(rec, P, acc0, cov, x2, rinv, accumulate=i > 0, sample_x2=sx[lo:hi] if samples else None,
                                    sample_expect=se[lo:hi] if samples else None, sample_terms=stm[lo:hi] if samples else None)
            lo = hi
        z = torch.empty((2, 4, P), dtype=torch.float64, device=d)
        phi = torch.empty((2, 4, P), dtype=torch.float32, device=d)
        status = torch.empty((2, 4, P), dtype=torch.uint8, device=d)
        counts = torch.zeros((4,), dtype=torch.int64, device=d)
        self.dispersion_finalize(P, acc0, x2, rinv, z_cutoff, z, phi, status, counts)
        return dict(x2=x2, rinv=rinv, z=z, phi=phi, status=status, counts=counts, sample_x2=sx, sample_expect=se, sample_terms=stm)

    def genotype_planes(self, rec: Records, P: int, min_depth: int = 100, absent_max_pm: int = 100, het_min_pm: int = 250, het_max_pm: int = 750,
                        hom_min_pm: int = 900, out=None):
        """Genotype bit planes of one resident chunk from its counts alone (ampli_genotype_planes_records): int64 [n, 6, W]
        holding the uint64 bit patterns, W = ceil(P / 64), planes V, A, C, G, T, H; bit i of word w is position 64 w + i.  Only the
        primary records enter.  out: the chunk's rows of a larger buffer (a contiguous int64 [n, 6, W] view), overwritten."""
        import torch

        n, W = rec.n_samples, int(self.lib.ampli_concordance_words(P))
        out = self._out(out, torch.int64, (n, GENO_PLANES, W))
        prm = GenotypeParams(min_depth, absent_max_pm, het_min_pm, het_max_pm, hom_min_pm)
        self._check(self.lib.ampli_genotype_planes_records(self.h, C.byref(rec), P, C.byref(prm), _ptr(out)))
        return out

    def concordance(self, planes_a, planes_b, P: int):
        """The five counts of every pair of two sets of genotype planes (ampli_concordance_pairs): int32 [n_a, n_b, 5] = sites, match,
        ibs0, het_either, het_match (CONC_*).  The same tensor twice: the set against itself, its upper triangle computed and mirrored."""
        import torch

        W = int(self.lib.ampli_concordance_words(P))
        assert _ok(planes_a, torch.int64, (None, GENO_PLANES, W)) and _ok(planes_b, torch.int64, (None, GENO_PLANES, W))
        n_a, n_b = planes_a.shape[0], planes_b.shape[0]
        out = torch.empty((n_a, n_b, 5), dtype=torch.int32, device=self.device)
        self._check(self.lib.ampli_concordance_pairs(self.h, P, _ptr(planes_a), n_a, _ptr(planes_b), n_b, _ptr(out)))
        return out

    def contamination(self, rec: Records, P: int, planes_a, planes_b, out=None):
        """The nine sums of every ordered pair (recipient of one resident chunk, source) of the cross-sample contamination check
        (ampli_contamination_records): int64 [n, n_b, 9] (CONTAM_*).  planes_a: the genotype planes of the chunk's own rows,
        int64 [n, 6, W]; planes_b: those of the n_b sources.  Only the primary records enter.  out: the chunk's rows of a larger matrix
        (a contiguous int64 [n, n_b, 9] view), overwritten."""
        import torch

        n, W = rec.n_samples, int(self.lib.ampli_concordance_words(P))
        assert _ok(planes_a, torch.int64, (None, GENO_PLANES, W)) and _ok(planes_b, torch.int64, (None, GENO_PLANES, W))
        assert planes_a.shape[0] == n
        n_b = planes_b.shape[0]
        out = self._out(out, torch.int64, (n, n_b, CONTAM_SUMS))
        self._check(self.lib.ampli_contamination_records(self.h, C.byref(rec), P, _ptr(planes_a), _ptr(planes_b), n_b, _ptr(out)))
        return out

    def amplicon_depth(self, rec: Records, P: int, amp_off, amp_pos, cov: int = 100, out=None):
        """The four depth sums (AMP_*) of every (sample of one resident chunk, amplicon): int64 [n, A, 4] (ampli_amplicon_depth_records,
        DESIGN 16).  amp_off [A + 1] and amp_pos [W] are the amplicons' position lists, a CSR over the BED walk with entries in [0, P):
        device int32 tensors (read as uint32) or host arrays, which are checked (monotone, in range) and uploaded.  Only the primary
        records enter.  out: the chunk's rows of a larger matrix (a contiguous int64 [n, A, 4] view), overwritten."""
        import torch

        amp_off, amp_pos, W = self._csr(amp_off, amp_pos, 1 << 28, P)
        n, A = rec.n_samples, amp_off.numel() - 1
        out = self._out(out, torch.int64, (n, A, AMP_SUMS))
        self._check(self.lib.ampli_amplicon_depth_records(self.h, C.byref(rec), P, A, _ptr(amp_off), _ptr(amp_pos), W, cov, _ptr(out)))
        return out

    def amplicon_reference(self, sums, use, min_normals: int = 5):
        """The reference of the panel of normals from their depth sums (int64 [N, A, 4]) and the mask use (uint8 [A]: the amplicons that
        count towards library size): dict of total int64 [N], med and mad float64 [A], status uint8 [A] (AMPLICON_*)
        (ampli_amplicon_reference)."""
        import torch

        assert _ok(sums, torch.int64, (None, None, AMP_SUMS))
        N, A = sums.shape[0], sums.shape[1]
        assert _ok(use, torch.uint8, (A,))
        total = torch.empty((N,), dtype=torch.int64, device=self.device)
        ref = torch.empty((A, 2), dtype=torch.float64, device=self.device)
        status = torch.empty((A,), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ampli_amplicon_reference(self.h, _ptr(sums), N, A, _ptr(use), min_normals, _ptr(total), _ptr(ref), _ptr(status)))
        return {"total": total, "med": ref[:, 0], "mad": ref[:, 1], "status": status, "ref": ref}

    def amplicon_ratio(self, sums, use, ref):
        """The ratios of any set of samples (int64 [S, A, 4] depth sums) against a reference (the dict of amplicon_reference): dict of
        total int64 [S], centre float64 [S], k int32 [S], ratio and z float64 [S, A] (ampli_amplicon_ratio)."""
        import torch

        assert _ok(sums, torch.int64, (None, None, AMP_SUMS))
        S, A = sums.shape[0], sums.shape[1]
        assert _ok(use, torch.uint8, (A,))
        r, st = ref["ref"], ref["status"]
        assert _ok(r, torch.float64, (A, 2)) and _ok(st, torch.uint8, (A,))
        total = torch.empty((S,), dtype=torch.int64, device=self.device)
        centre = torch.empty((S,), dtype=torch.float64, device=self.device)
        k = torch.empty((S,), dtype=torch.int32, device=self.device)
        ratio = torch.empty((S, A), dtype=torch.float64, device=self.device)
        z = torch.empty((S, A), dtype=torch.float64, device=self.device)
        self._check(self.lib.ampli_amplicon_ratio(self.h, _ptr(sums), S, A, _ptr(use), _ptr(r), _ptr(st), _ptr(total), _ptr(centre), _ptr(k),
                                                  _ptr(ratio), _ptr(z)))
        return {"total": total, "centre": centre, "k": k, "ratio": ratio, "z": z}

    def spectrum(self, rec: Records, P: int, ref_code, cls, C: int, cov: int = 100, max_alt_pm: int = 30, out=None):
        """The nine class sums (SPEC_*) of every (sample of one resident chunk, class): int64 [n, C, 9] (ampli_spectrum_records).
        ref_code and cls are uint8 [P]: the reference code (0..3) and the class (below C, or anything from C up -- 255 by convention --
        to skip the position) of every position; device uint8 tensors, or host arrays, which are checked and uploaded.  Only the
        primary records enter.  out: the chunk's rows of a larger matrix (a contiguous int64 [n, C, 9] view), overwritten."""
        import ctypes  # the module's alias C is this method's number of classes

        import torch

        ref_code, cls = self._positions_u8(ref_code, P), self._positions_u8(cls, P)
        out = self._out(out, torch.int64, (rec.n_samples, C, SPEC_SUMS))
        self._check(self.lib.ampli_spectrum_records(self.h, ctypes.byref(rec), P, _ptr(ref_code), _ptr(cls), C, cov, max_alt_pm, _ptr(out)))
        return out

    def last_spectrum_segments(self) -> int:
        """the number of position segments the last spectrum() launch was cut into (ampli_last_spectrum_segments)"""
        return int(self.lib.ampli_last_spectrum_segments(self.h))

    def exceedance(self, tumours: Records, normals: Records, P: int, ref_code, normal_cutoff: int = 100, calling_cutoff: int = 100, first_t: int = 0,
                   first_n: int = 0, skip_same_index: bool = False, accumulate: bool = False, elig=None, ge=None):
        """How many normals of one resident chunk reach every tumour row of another at every (position, base, strand)
        (ampli_exceedance_records): (elig int16 [n_t, P], ge int16 [n_t, P, 4, 2]), to be read as unsigned 16-bit counts
        (torch has no arithmetic on uint16: .cpu().numpy().view(numpy.uint16)); a cell of ge that is not evaluated holds EXCEEDANCE_NA.
        ref_code is uint8 [P], a device tensor or a host array.  first_t, first_n: the global indices of the chunks' first rows;
        skip_same_index leaves out the normal with a tumour row's own global index.  accumulate adds this chunk's normals onto the
        elig and ge of the earlier chunks, which must then be given."""
        import ctypes

        import torch

        ref_code = self._positions_u8(ref_code, P)
        n_t = tumours.n_samples
        assert not accumulate or (elig is not None and ge is not None), "accumulate adds onto the outputs of the earlier chunks"
        elig = self._out(elig, torch.int16, (n_t, P))
        ge = self._out(ge, torch.int16, (n_t, P, 4, 2))
        self._check(self.lib.ampli_exceedance_records(self.h, ctypes.byref(tumours), ctypes.byref(normals), P, _ptr(ref_code), normal_cutoff, calling_cutoff,
                                                      first_t, first_n, int(bool(skip_same_index)), int(bool(accumulate)), _ptr(elig), _ptr(ge)))
        return elig, ge

    def overdispersion_sums(self, chunks, P: int, acc0: Acc, cov: int = 100, s2=None, accumulate: bool = False):
        """S2 = sum of d_i^2 over every cell's qualifying records (ampli_overdispersion_records): float64 [2, 4, P].
        chunks: one Records or the Records of the resident cohort in visit order; acc0: the cohort's C_value = 0 table of P positions.
        accumulate adds onto an s2 of earlier chunks, which must then be given."""
        import torch

        if isinstance(chunks, Records):
            chunks = [chunks]
        assert not accumulate or s2 is not None, "accumulate adds onto the sums of the earlier chunks"
        s2 = self._out(s2, torch.float64, (2, 4, P))
        for i, rec in enumerate(chunks):
            self._check(self.lib.ampli_overdispersion_records(self.h, C.byref(rec), P, C.byref(acc0.struct), cov, _ptr(s2),
                                                              int(bool(accumulate) or i > 0)))
        return s2

    def overdispersion_fit(self, P: int, acc0: Acc, x2, s2, status, omega=None):
        """omega float64 [2, 4, P] from dispersion's x2 and status (panel_dispersion) and s2 (overdispersion_sums)
        (ampli_overdispersion_finalize): 0 in every cell that is not DISPERSION_HIGH."""
        import torch

        omega = self._out(omega, torch.float64, (2, 4, P))
        assert _ok(x2, torch.float64, (2, 4, P)) and _ok(s2, torch.float64, (2, 4, P)) and _ok(status, torch.uint8, (2, 4, P))
        self._check(self.lib.ampli_overdispersion_finalize(self.h, P, C.byref(acc0.struct), _ptr(x2), _ptr(s2), _ptr(status), _ptr(omega)))
        return omega

    def nb_score(self, tumours: Records, P: int, thr, ref_code, omega=None, calling_cutoff: int = 100, q=None):
        """The negative-binomial score of every cell of a resident chunk of tumours (ampli_nb_score_records): q float32
        [n_t, P, 4, 2] per base and strand, NB_NA (-1) in a cell that is not evaluated.  thr: the error table's float32 [2, 4, P];
        omega: float64 [2, 4, P] of overdispersion_fit, or None for 0 everywhere -- the exact Poisson tail; ref_code: uint8 [P]."""
        import torch

        n_t = tumours.n_samples
        q = self._out(q, torch.float32, (n_t, P, 4, 2))
        assert _ok(thr, torch.float32) and thr.numel() == 8 * P
        assert omega is None or (_ok(omega, torch.float64) and omega.numel() == 8 * P)
        assert _ok(ref_code, torch.uint8, (P,))
        self._check(self.lib.ampli_nb_score_records(self.h, C.byref(tumours), P, _ptr(thr), _ptr(omega), _ptr(ref_code), calling_cutoff, _ptr(q)))
        return q

    def pair_score(self, recs_a: Records, recs_b: Records, P: int, pairs, ref_code, depth_cutoff: int = 100, s=None):
        """The exact conditional test of two count files at every cell (ampli_pair_score_records): s float32
        [n_pairs, P, 4, 2] per base and strand, positive where a's allele fraction is the higher, PAIR_NA (-999) in a cell that is not
        evaluated.  pairs: int32 [n_pairs, 2] on the device, a row of recs_a and a row of recs_b (which may be the same chunk); a row
        index outside its chunk makes the pair all NA.  ref_code: uint8 [P]."""
        import torch

        assert _ok(pairs, torch.int32, (None, 2))
        n_pairs = int(pairs.shape[0])
        s = self._out(s, torch.float32, (n_pairs, P, 4, 2))
        assert _ok(ref_code, torch.uint8, (P,))
        self._check(self.lib.ampli_pair_score_records(self.h, C.byref(recs_a), C.byref(recs_b), P, _ptr(pairs), n_pairs, _ptr(ref_code),
                                                      depth_cutoff, _ptr(s)))
        return s

    def dilute(self, recs_a: Records, recs_b: Records | None, P: int, mixtures, out=None, flags=None):
        """In-silico dilution (ampli_dilute_records): every mixture thins row_a of recs_a and, unless row_b is -1, row_b of
        recs_b read by read and adds the two.  mixtures: a sequence of (row_a, row_b, keep_a, keep_b, key) -- keep in [0, 2^32] is the
        threshold of ampli_host_dilute_keep, key any 64-bit word -- or a device tensor of descriptors (uint8 [n_mix, 32] or int64
        [n_mix, 4]).  Returns (out, flags): out int32 [n_mix, P, 8], dense records of the I32 layout (dilution_records wraps them), flags
        int32 [n_mix] (DILUTE_BAD_COUNT, DILUTE_BAD_MIXTURE)."""
        import torch

        if isinstance(mixtures, torch.Tensor):
            d_mix = mixtures
            assert d_mix.is_cuda and d_mix.is_contiguous() and d_mix.dim() == 2 and d_mix.shape[1] * d_mix.element_size() == C.sizeof(DiluteMix)
        else:
            if not len(mixtures):
                raise AmpliError("dilute: the list of mixtures is empty")
            rows = [DiluteMix(int(ra), int(rb), int(ka), int(kb), int(key) & 0xFFFFFFFFFFFFFFFF) for ra, rb, ka, kb, key in mixtures]
            host = torch.frombuffer(bytearray(bytes((DiluteMix * len(rows))(*rows))), dtype=torch.uint8)
            d_mix = host.view(len(rows), C.sizeof(DiluteMix)).to(self.device)
        n_mix = int(d_mix.shape[0])
        out = self._out(out, torch.int32, (n_mix, P, 8))
        flags = self._out(flags, torch.int32, (n_mix,))
        self._check(self.lib.ampli_dilute_records(self.h, C.byref(recs_a), C.byref(recs_b) if recs_b is not None else None, P, _ptr(d_mix), n_mix,
                                                  _ptr(out), _ptr(flags)))
        return out, flags

    def _monitor_lists(self, P: int, thr, ref_code, list_off, list_cell):
        """the arguments the two monitoring gathers share: (thr, ref_code, list_off, list_cell, L, W) on the device.  Host lists are
        checked (monotone offsets, cells that fit 32 bits -- an entry at or beyond P is none, by the definition) and uploaded; device lists
        are taken as they are (the kernels cut them)."""
        import torch

        list_off, list_cell, W = self._csr(list_off, list_cell, 1 << 28, 1 << 32)
        assert _ok(thr, torch.float32) and thr.numel() == 8 * P
        assert _ok(ref_code, torch.uint8, (P,))
        return thr, ref_code, list_off, list_cell, list_off.numel() - 1, W

    def monitor_sums(self, rec: Records, P: int, thr, ref_code, list_off, list_cell, cov: int = 100, max_vaf_pm: int = 1000, sums=None, lam=None):
        """The pooled sums of every (sample of one resident chunk, variant list) (ampli_monitor_sums_records): sums int64
        [n, L, 6] (MON_*) and lam float64 [n, L, 2], the expected counts of the strands under the error table.  thr: the table's
        float32 [2, 4, P]; ref_code uint8 [P]; list_off [L + 1] and list_cell [W]: the lists as a CSR of cells 4 p + y -- device int32
        tensors (read as uint32) or host arrays.  sums, lam: the chunk's rows of larger matrices (contiguous views), overwritten."""
        import torch

        thr, ref_code, list_off, list_cell, L, W = self._monitor_lists(P, thr, ref_code, list_off, list_cell)
        n = rec.n_samples
        sums = self._out(sums, torch.int64, (n, L, MON_SUMS))
        lam = self._out(lam, torch.float64, (n, L, 2))
        prm = MonitorParams(int(cov), int(max_vaf_pm))
        self._check(self.lib.ampli_monitor_sums_records(self.h, C.byref(rec), P, _ptr(thr), _ptr(ref_code), _ptr(list_off), _ptr(list_cell), L, W,
                                                        C.byref(prm), _ptr(sums), _ptr(lam)))
        return sums, lam

    def monitor_controls(self, rec: Records, P: int, thr, ref_code, list_off, list_cell, pairs, cand_off, cand_pos, R: int, first_rep: int = 0,
                         seed: int = 0, cov: int = 100, max_vaf_pm: int = 1000, sums=None, lam=None):
        """The sums of R matched random control lists for every (row, list) of pairs (ampli_monitor_control_records): every
        entry of the list is moved to a position drawn among the candidates of its reference base (cand_off int32 [5], cand_pos int32
        [n_cand] on the device: positions grouped by reference base), replicates first_rep .. first_rep + R - 1 of seed.  pairs: int32
        [n_pairs, 2] on the device; a row or list outside its range gives zeros.  Returns sums int64 [n_pairs, R, 6] and lam float64
        [n_pairs, R, 2]; a replicate's cells do not depend on the batch it is computed in."""
        import torch

        thr, ref_code, list_off, list_cell, L, W = self._monitor_lists(P, thr, ref_code, list_off, list_cell)
        assert _ok(pairs, torch.int32, (None, 2))
        assert _ok(cand_off, torch.int32, (5,)) and _ok(cand_pos, torch.int32, (None,))
        n_pairs, n_cand = int(pairs.shape[0]), int(cand_pos.numel())
        if n_cand == 0:
            cand_pos = torch.zeros((1,), dtype=torch.int32, device=self.device)
        sums = self._out(sums, torch.int64, (n_pairs, R, MON_SUMS))
        lam = self._out(lam, torch.float64, (n_pairs, R, 2))
        prm = MonitorParams(int(cov), int(max_vaf_pm))
        self._check(self.lib.ampli_monitor_control_records(self.h, C.byref(rec), P, _ptr(thr), _ptr(ref_code), _ptr(list_off), _ptr(list_cell), L, W,
                                                           _ptr(pairs), n_pairs, _ptr(cand_off), _ptr(cand_pos), n_cand, R, first_rep,
                                                           int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(prm), _ptr(sums), _ptr(lam)))
        return sums, lam

    def monitor_score(self, sums, lam, q=None):
        """The pooled Poisson score of both strands of every cell of monitor_sums or monitor_controls (ampli_monitor_score):
        float32 [..., 2], MON_NA (-1) where no entry was evaluated."""
        import torch

        assert _ok(sums, torch.int64, (..., MON_SUMS))
        assert _ok(lam, torch.float64, tuple(sums.shape[:-1]) + (2,))
        q = self._out(q, torch.float32, tuple(lam.shape))
        self._check(self.lib.ampli_monitor_score(self.h, _ptr(sums), _ptr(lam), sums.numel() // MON_SUMS, _ptr(q)))
        return q

    def tumour_fraction(self, rec: Records, P: int, thr, ref_code, list_off, list_cell, list_w, cov: int = 100, max_vaf_pm: int = 1000,
                        z2: float = None, est=None, count=None):
        """The tumour fraction of every (sample of one resident chunk, weighted variant list) (ampli_fraction_records): est
        float64 [n, L, 4] (TF_F_HAT, TF_F_LO, TF_F_HI, TF_T0: the score estimate, the ends of its Rao score interval at the squared normal
        quantile z2 -- TF_Z2_95 by default -- and the signed squared score at zero; all TF_NA where nothing can be estimated) and count
        int64 [n, L, 2] (TF_N_EVAL, TF_N_SEEN).  thr, ref_code, list_off, list_cell as monitor_sums takes them; list_w: float32 [W], the
        weight of every entry in (0, 1] -- a device tensor, or a host array, which is uploaded.  est, count: the chunk's rows of larger
        matrices (contiguous views), overwritten."""
        import numpy as np
        import torch

        thr, ref_code, list_off, list_cell, L, W = self._monitor_lists(P, thr, ref_code, list_off, list_cell)
        if not isinstance(list_w, torch.Tensor):
            w = np.ascontiguousarray(list_w, np.float32)
            list_w = torch.from_numpy(w if len(w) else np.zeros(1, np.float32)).to(self.device)
        elif list_w.numel() == 0:  # a pointer is required even where nothing is read through it
            list_w = torch.zeros((1,), dtype=torch.float32, device=self.device)
        assert _ok(list_w, torch.float32, (None,)) and list_w.numel() >= W
        n = rec.n_samples
        est = self._out(est, torch.float64, (n, L, TF_VALS))
        count = self._out(count, torch.int64, (n, L, TF_COUNTS))
        prm = FractionParams(int(cov), int(max_vaf_pm), float(TF_Z2_95 if z2 is None else z2))
        self._check(self.lib.ampli_fraction_records(self.h, C.byref(rec), P, _ptr(thr), _ptr(ref_code), _ptr(list_off), _ptr(list_cell), _ptr(list_w), L, W,
                                                    C.byref(prm), _ptr(est), _ptr(count)))
        return est, count

    def indel_count(self, bam, rec_off, keys, mbq: int = 20, mrq: int = 20, counts=None, lengths=None, stats=None):
        """Indel junction counts of a batch of alignment records (ampli_pileup_indel_count).  bam: uint8 device tensor, the
        uncompressed records, 16-byte aligned and readable for 16 bytes behind the last record; rec_off: int64 [n_reads], ascending
        offsets of the records' block_size fields; keys: int64 [P], the panel as (reference id << 32 | 1-based position), ascending.
        Returns (counts, lengths, stats): counts int32 [P, 8] (slot 0 reference junctions, 1 insertions, 2 deletions, 4..6 the same on the
        reverse strand; 3 and 7 untouched), lengths int32 [P, 2, INDEL_LEN_BINS] and stats int64 [2] (reads kept, junctions counted).
        All three are ADDED TO: a given buffer accumulates, None starts a new one at zero; lengths=False / stats=False: that output is
        not computed (NULL) and returned as None."""
        import torch

        assert _ok(bam, torch.uint8, (None,)) and bam.data_ptr() % 16 == 0 and _ok(rec_off, torch.int64, (None,)) and _ok(keys, torch.int64, (None,))
        n_reads, P = int(rec_off.numel()), int(keys.numel())
        counts = self._out(counts, torch.int32, (P, 8), zero=True)
        lengths = None if lengths is False else self._out(lengths, torch.int32, (P, 2, INDEL_LEN_BINS), zero=True)
        stats = None if stats is False else self._out(stats, torch.int64, (2,), zero=True)
        self._check(self.lib.ampli_pileup_indel_count(self.h, _ptr(bam), _ptr(rec_off), n_reads, _ptr(keys), P, int(mbq), int(mrq), _ptr(counts), _ptr(lengths),
                                                      _ptr(stats)))
        return counts, lengths, stats

    def _amplicons(self, lo, hi, reach, amp_off, counts):
        """the four sorted amplicon arrays of amplicon_count / amplicon_layers, checked: (lo, hi, reach, amp_off, A, W).  W is the rows of
        `counts` where the caller has them (no read-back), amp_off[A] otherwise.  A pointer is required even where nothing is read
        through it (A = 0)."""
        import torch

        A = int(lo.numel())
        assert _ok(lo, torch.int64, (A,)) and _ok(hi, torch.int64, (A,)) and _ok(reach, torch.int64, (A,)) and _ok(amp_off, torch.int64, (A + 1,))
        W = int(counts.shape[0]) if counts is not None else int(amp_off[-1])
        if A == 0:
            lo = hi = reach = torch.zeros((1,), dtype=torch.int64, device=self.device)
        return lo, hi, reach, amp_off, A, W

    def amplicon_count(self, bam, rec_off, lo, hi, reach, amp_off, mbq: int = 20, mrq: int = 20, min_overlap: int = 50, counts=None, amp_reads=None,
                       stats=None):
        """Amplicon-resolved counts of a batch of alignment records (ampli_pileup_amplicon_count): every kept read is assigned
        to one amplicon and counted inside it only.  bam, rec_off as indel_count takes them; lo, hi, reach: int64 [A], the amplicons as
        (reference id << 32 | first / last position), sorted by lo then hi, and the running maximum of hi; amp_off: int64 [A + 1], the
        exclusive prefix sum of their lengths (amp_off[A] = W).  Returns (counts, amp_reads, stats): counts int32 [W, 8] per walk entry
        amp_off[a] + (x - first[a]), amp_reads int64 [A, 2] (assigned forward and reverse reads) and stats int64 [4] (reads kept, reads
        assigned, bases counted, bases clipped).  All three are ADDED TO: a given buffer accumulates, None starts a new one at zero;
        stats=False: not computed (NULL) and returned as None."""
        import torch

        assert _ok(bam, torch.uint8, (None,)) and _ok(rec_off, torch.int64, (None,))
        lo, hi, reach, amp_off, A, W = self._amplicons(lo, hi, reach, amp_off, counts)
        counts = self._out(counts, torch.int32, (W, 8), zero=True)
        amp_reads = self._out(amp_reads, torch.int64, (A, 2), zero=True)
        stats = None if stats is False else self._out(stats, torch.int64, (4,), zero=True)
        self._check(self.lib.ampli_pileup_amplicon_count(self.h, _ptr(bam), _ptr(rec_off), int(rec_off.numel()), _ptr(lo), _ptr(hi), _ptr(reach), _ptr(amp_off), A, W,
                                                         int(mbq), int(mrq), int(min_overlap), _ptr(counts), _ptr(amp_reads), _ptr(stats)))
        return counts, amp_reads, stats

    def amplicon_layers(self, counts, lo, hi, reach, amp_off, keys, L: int = 2, layers=None, layer_amp=None, total=None):
        """The counts of amplicon_count gathered per listed position (ampli_amplicon_layers).  keys: int64 [P], positions as
        (reference id << 32 | 1-based position), any order, repeats allowed.  Returns (layers, layer_amp, total): layers int32 [L, P, 8],
        the record of the l-th amplicon over the position in sorted order (slot 0 = INT32_MIN, the rest 0, where there is none);
        layer_amp int32 [L, P], that amplicon's sorted index or -1; total int32 [P, 8], the sum over all amplicons over the position.
        All three are overwritten."""
        import torch

        lo, hi, reach, amp_off, A, W = self._amplicons(lo, hi, reach, amp_off, counts)
        P = int(keys.numel())
        assert _ok(keys, torch.int64, (P,)) and _ok(counts, torch.int32, (W, 8))
        layers = self._out(layers, torch.int32, (L, P, 8))
        layer_amp = self._out(layer_amp, torch.int32, (L, P))
        total = self._out(total, torch.int32, (P, 8))
        self._check(self.lib.ampli_amplicon_layers(self.h, _ptr(counts), _ptr(lo), _ptr(hi), _ptr(reach), _ptr(amp_off), A, W, _ptr(keys), P, int(L), _ptr(layers),
                                                   _ptr(layer_amp), _ptr(total)))
        return layers, layer_amp, total

    def read_evidence(self, bam, rec_off, keys, mbq: int = 20, mrq: int = 20, hist=None, stats=None):
        """Read-level evidence of a batch of alignment records (ampli_pileup_evidence).  bam, rec_off, keys as indel_count takes
        them.  Returns (hist, stats): hist int32 [P, 4, EVIDENCE_METRICS, EVIDENCE_BINS] in the order (position, nt, metric, bin) -- per
        counted column one count in the bin of its base quality (EVIDENCE_BQ), its read's MAPQ / 4 (EVIDENCE_MQ) and its distance to the
        nearer end of the read (EVIDENCE_POS), each clamped at 63 -- and stats int64 [2] (reads kept, columns counted).  Both are ADDED TO:
        a given buffer accumulates, None starts a new one at zero; stats=False: not computed (NULL) and returned as None."""
        import torch

        assert _ok(bam, torch.uint8, (None,)) and _ok(rec_off, torch.int64, (None,)) and _ok(keys, torch.int64, (None,))
        n_reads, P = int(rec_off.numel()), int(keys.numel())
        hist = self._out(hist, torch.int32, (P, 4, EVIDENCE_METRICS, EVIDENCE_BINS), zero=True)
        stats = None if stats is False else self._out(stats, torch.int64, (2,), zero=True)
        self._check(self.lib.ampli_pileup_evidence(self.h, _ptr(bam), _ptr(rec_off), n_reads, _ptr(keys), P, int(mbq), int(mrq), _ptr(hist), _ptr(stats)))
        return hist, stats

    def evidence_score(self, hist, ref_nt, alt_nt, ints=None, med=None, z2=None, alt_used=None):
        """The rank-sum score of alt reads against ref reads per (position, metric) of read_evidence's histograms (ampli_evidence_score,
        DESIGN 29).  ref_nt, alt_nt: int8 [P], 0 .. 3 = A C G T; an alt of -1 takes the non-reference nt with the most reads.  Returns
        (ints, med, z2, alt_used): ints int64 [P, 3, 3] (n_ref, n_alt, u2; u2 = -1: untested), med int32 [P, 3, 2] (median bin of the ref
        and of the alt reads, -1 without reads), z2 float64 [P, 3] (the signed squared normal score, < 0: alt ranks below ref) and alt_used
        int8 [P].  All four are overwritten."""
        import torch

        P = int(hist.shape[0])
        assert _ok(hist, torch.int32, (P, 4, EVIDENCE_METRICS, EVIDENCE_BINS)) and _ok(ref_nt, torch.int8, (P,)) and _ok(alt_nt, torch.int8, (P,))
        ints = self._out(ints, torch.int64, (P, EVIDENCE_METRICS, 3))
        med = self._out(med, torch.int32, (P, EVIDENCE_METRICS, 2))
        z2 = self._out(z2, torch.float64, (P, EVIDENCE_METRICS))
        alt_used = self._out(alt_used, torch.int8, (P,))
        self._check(self.lib.ampli_evidence_score(self.h, _ptr(hist), P, _ptr(ref_nt), _ptr(alt_nt), _ptr(ints), _ptr(med), _ptr(z2), _ptr(alt_used)))
        return ints, med, z2, alt_used

    def hetsite_reference(self, rec: Records, P: int, planes, min_depth: int = 100, ref=None):
        """One resident chunk of normals into the het-site reference (ampli_hetsite_reference_records): ref int64 [3, 6, P]
        (AI_REF_CNT / _LO / _HI per pair code and position) is ADDED TO -- a new one starts at zero, streamed chunks accumulate.  planes:
        the genotype planes of the chunk's own rows, int64 [n, 6, W].  Only the primary records enter."""
        import torch

        n, W = rec.n_samples, int(self.lib.ampli_concordance_words(P))
        assert _ok(planes, torch.int64, (n, GENO_PLANES, W))
        ref = self._out(ref, torch.int64, (3, 6, P), zero=True)
        self._check(self.lib.ampli_hetsite_reference_records(self.h, C.byref(rec), P, _ptr(planes), int(min_depth), _ptr(ref)))
        return ref

    def allelic_sites(self, rec: Records, P: int, planes_g, row_g, ref, min_depth: int = 100, min_normals: int = 5, half_fallback: bool = True,
                      q=None, km=None, v=None, code=None):
        """The allelic balance of every (sample of one resident chunk, position) at the het sites of the sample's germline
        (ampli_allelic_site_records).  planes_g: genotype planes int64 [n_g, 6, W]; row_g: int32 [n] on the device, the plane row
        of each sample's germline (outside [0, n_g): none); ref: the het-site reference int64 [3, 6, P].  Returns q float32 [n, P]
        (signed score, AI_NA where untested), km int32 [n, P, 2] (k_lo, m), v float64 [n, P] (the expected share) and code uint8 [n, P]
        (status * 8 + pair); given buffers (the chunk's rows of larger planes) are overwritten."""
        import torch

        n, W = rec.n_samples, int(self.lib.ampli_concordance_words(P))
        assert _ok(planes_g, torch.int64, (None, GENO_PLANES, W)) and _ok(row_g, torch.int32, (n,)) and _ok(ref, torch.int64, (3, 6, P))
        q, km = self._out(q, torch.float32, (n, P)), self._out(km, torch.int32, (n, P, 2))
        v, code = self._out(v, torch.float64, (n, P)), self._out(code, torch.uint8, (n, P))
        prm = AllelicParams(int(min_depth), int(min_normals), int(bool(half_fallback)))
        self._check(self.lib.ampli_allelic_site_records(self.h, C.byref(rec), P, _ptr(planes_g), int(planes_g.shape[0]), _ptr(row_g), _ptr(ref),
                                                        C.byref(prm), _ptr(q), _ptr(km), _ptr(v), _ptr(code)))
        return q, km, v, code

    def allelic_regions(self, q, km, v, code, reg_off, reg_pos, site_q: float = 20.0, out=None):
        """The five sums (AI_*) of every (sample, region) over the site planes of allelic_sites (ampli_allelic_region_sums):
        int64 [S, R, 5].  reg_off [R + 1] and reg_pos [W]: the regions' position lists as a CSR -- device int32 tensors (read as uint32)
        or host arrays, which are checked (monotone offsets, entries that fit 32 bits; an entry at or beyond P is none) and uploaded."""
        import torch

        S, P = int(q.shape[0]), int(q.shape[1])
        assert _ok(q, torch.float32, (S, P)) and _ok(km, torch.int32, (S, P, 2)) and _ok(v, torch.float64, (S, P)) and _ok(code, torch.uint8, (S, P))
        reg_off, reg_pos, W = self._csr(reg_off, reg_pos, 1 << 27, 1 << 32)
        R = reg_off.numel() - 1
        out = self._out(out, torch.int64, (S, R, AI_SUMS))
        self._check(self.lib.ampli_allelic_region_sums(self.h, _ptr(q), _ptr(km), _ptr(v), _ptr(code), S, P, R, _ptr(reg_off), _ptr(reg_pos), W,
                                                       float(site_q), _ptr(out)))
        return out

    def dilution_records(self, out) -> Records:
        """the mixtures dilute wrote as Records (I32, dense, E = 0, a row per mixture): what detection_limits, nb_score and the others take"""
        return self.records(out, "i32", int(out.shape[0]))

    def fdr_workspace_bytes(self, rows: int, P: int) -> int:
        """Bytes of the workspace fdr_adjust needs for a plane of rows x P positions (ampli_fdr_workspace_bytes)."""
        return int(self.lib.ampli_fdr_workspace_bytes(rows, P))

    def fdr_adjust(self, s, two_sided: bool = False, a=None, m=None, rank=False, work=None):
        """The Benjamini-Hochberg adjusted score of every cell of a score plane, each row on its own (ampli_fdr_adjust).
        s: float32 [rows, P, 4, 2] of nb_score (two_sided False) or pair_score (two_sided True).  Returns (a, m) or, with rank (True,
        or an int32 [rows, P, 4] tensor to fill), (a, m, rank): a float32 [rows, P, 4] -- the signed adjusted score, FDR_NA (-999) in a
        cell that is not tested --, m int32 [rows] the tested cells of each row, rank the cell's rank R among them.  work: a uint8
        tensor of at least fdr_workspace_bytes(rows, P) bytes; allocated here when not given."""
        import torch

        assert _ok(s, torch.float32, (None, None, 4, 2))
        rows, P = int(s.shape[0]), int(s.shape[1])
        a = self._out(a, torch.float32, (rows, P, 4))
        m = self._out(m, torch.int32, (rows,))
        if rank is True:
            rank = torch.empty((rows, P, 4), dtype=torch.int32, device=self.device)
        elif rank is False:
            rank = None
        if work is None:
            work = torch.empty((self.fdr_workspace_bytes(rows, P),), dtype=torch.uint8, device=self.device)
        assert rank is None or _ok(rank, torch.int32, (rows, P, 4))
        assert _ok(work, torch.uint8)
        self._check(self.lib.ampli_fdr_adjust(self.h, _ptr(s), rows, P, int(bool(two_sided)), _ptr(work), work.numel(), _ptr(a), _ptr(m), _ptr(rank)))
        return (a, m) if rank is None else (a, m, rank)

    def loo_call(self, rec: Records, P: int, acc: Acc, ref_code, C_value: float = 0.002, cov: int = 100, call_cov: int = 100,
                 mode: int = POISSON_PREFILTER, capacity: int = 0, dense_thr: bool = False, call_mask=None, calls_buf=None,
                 n_calls=None, callable_pos=None, callable_sample=None, flags=None, thr_loo=None):
        """Leave-one-out calls of one resident chunk of the panel of normals (ampli_loo_call_records): every normal of the chunk
        through the calling gate (calling cutoff call_cov) against the error table (C_value, cov) of the cohort without it.  acc holds
        the WHOLE cohort's sums.  callable_pos [P] / callable_sample [n] are added to (zeroed here when not given); flags[0] gets bit 0
        when a total is outside the exactness envelope.  dense_thr: also the S-1 thresholds, float32 [n, 2, 4, P] (into thr_loo when
        the caller brings the buffer)."""
        import torch

        n, R = rec.n_samples, P + rec.E
        d = self.device
        call_mask, calls_buf, capacity, n_calls = self._call_list(n, R, LooCall, capacity, call_mask, calls_buf, n_calls)
        if callable_pos is None:
            callable_pos = torch.zeros((P,), dtype=torch.int32, device=d)
        if callable_sample is None:
            callable_sample = torch.zeros((n,), dtype=torch.int32, device=d)
        if flags is None:
            flags = torch.zeros((1,), dtype=torch.int32, device=d)
        if thr_loo is None and dense_thr:
            thr_loo = torch.empty((n, 2, 4, P), dtype=torch.float32, device=d)
        self._check(self.lib.ampli_loo_call_records(self.h, C.byref(rec), P, C.byref(acc.struct), C_value, cov, call_cov, _ptr(ref_code), mode,
                                                    _ptr(call_mask), _ptr(calls_buf), capacity, _ptr(n_calls), _ptr(callable_pos),
                                                    _ptr(callable_sample), _ptr(thr_loo), _ptr(flags)))
        return dict(call_mask=call_mask, calls_buf=calls_buf, n_calls=n_calls, capacity=capacity, callable_pos=callable_pos,
                    callable_sample=callable_sample, thr_loo=thr_loo, flags=flags)

    def read_loo_calls(self, res):
        """The leave-one-out call list on the host, sorted by (sample, record, alt): the fields of read_calls + thr_fw, thr_bw, code."""
        return self._read_list(res, LooCall)

    def _new_error_table(self, P: int) -> ErrorTable:
        import torch

        d = self.device
        return ErrorTable(rate=torch.empty((2, 4, P), dtype=torch.float32, device=d),
                          code=torch.empty((4, P), dtype=torch.uint8, device=d),
                          thr=torch.empty((2, 4, P), dtype=torch.float32, device=d),
                          germ_val=torch.empty((4, P), dtype=torch.float32, device=d),
                          germ_present=torch.empty((4, P), dtype=torch.uint8, device=d),
                          flags=torch.zeros((1,), dtype=torch.int32, device=d))

    def error_estimate(self, recs, P: int, C_value: float = 0.002, cov: int = 100, E: int = 0, dup_off=None,
                       acc: Acc | None = None, out: ErrorTable | None = None) -> ErrorTable:
        """Fused error_reduce + error_finalize (ampli_error_estimate); acc optional."""
        import torch

        assert recs.dtype == self._rec_dtype() and recs.is_cuda and recs.is_contiguous()
        S = recs.shape[0]
        assert recs.numel() == S * (P + E) * self._rec_elems()
        if out is None:
            out = self._new_error_table(P)
        self._check(self.lib.ampli_error_estimate(self.h, _ptr(recs), P, E, _ptr(dup_off), S, C_value, cov,
                                                  C.byref(acc.struct) if acc is not None else None, _ptr(out.rate), _ptr(out.code),
                                                  _ptr(out.thr), _ptr(out.germ_val), _ptr(out.germ_present), _ptr(out.flags)))
        return out

    def error_reduce_packed(self, recs, P: int, acc: Acc, packed, C_value: float = 0.002, cov: int = 100, E: int = 0,
                            dup_off=None, first_sample: int = 0):
        """Shard reduction for the multi-GPU merge: additive planes -> packed (float64 [21*P]), gm planes -> acc."""
        S = recs.shape[0]
        self._check(self.lib.ampli_error_reduce_packed(self.h, _ptr(recs), P, E, _ptr(dup_off), S, first_sample, C_value, cov,
                                                       C.byref(acc.struct), _ptr(packed)))

    def error_finalize_merged(self, P: int, packed, gm_regions, nparts: int, C_value: float = 0.002, cov: int = 100,
                              out: ErrorTable | None = None) -> ErrorTable:
        if out is None:
            out = self._new_error_table(P)
        self._check(self.lib.ampli_error_finalize_merged(self.h, P, _ptr(packed), _ptr(gm_regions), nparts, C_value, cov,
                                                         _ptr(out.rate), _ptr(out.code), _ptr(out.thr), _ptr(out.germ_val),
                                                         _ptr(out.germ_present), _ptr(out.flags)))
        return out

    # ---- position-sliced merge (reduce-scatter / all-to-all / all-gather; include/amplisolve_hip.h) ----
    def set_slice_group(self, group_size: int = 1, group_index: int = 0):
        """The sliced exchange buffers hold group_size batches per slice chunk; the following sliced calls address batch
        group_index (include/amplisolve_hip.h, ampli_set_slice_group)."""
        self._check(self.lib.ampli_set_slice_group(self.h, group_size, group_index))

    def slice_len(self, P: int, n_slices: int) -> int:
        return int(self.lib.ampli_slice_len(P, n_slices))

    def error_reduce_sliced(self, recs, P: int, n_slices: int, sums, gm, C_value: float = 0.002, cov: int = 100, E: int = 0,
                            dup_off=None, first_sample: int = 0):
        """Shard reduction straight into the exchange buffers: sums f64 [n][21][L], gm f32 [n][8][L]."""
        S = recs.shape[0]
        self._check(self.lib.ampli_error_reduce_sliced(self.h, _ptr(recs), P, E, _ptr(dup_off), S, first_sample, C_value, cov,
                                                       n_slices, _ptr(sums), _ptr(gm)))

    def error_finalize_slice(self, P: int, n_slices: int, slice_index: int, sum_slice, gm_recv, block, C_value: float = 0.002,
                             cov: int = 100):
        self._check(self.lib.ampli_error_finalize_slice(self.h, P, n_slices, slice_index, _ptr(sum_slice), _ptr(gm_recv),
                                                        C_value, cov, _ptr(block)))

    def error_table_unslice(self, P: int, n_slices: int, blocks, out: ErrorTable | None = None) -> ErrorTable:
        if out is None:
            out = self._new_error_table(P)
        self._check(self.lib.ampli_error_table_unslice(self.h, P, n_slices, _ptr(blocks), _ptr(out.rate), _ptr(out.code),
                                                       _ptr(out.thr), _ptr(out.germ_val), _ptr(out.germ_present), _ptr(out.flags)))
        return out

    def acc_merge(self, parts: list[Acc], dst: Acc | None = None) -> Acc:
        if dst is None:
            dst = self.new_acc(parts[0].P)
        arr = (AccTable * len(parts))(*[p.struct for p in parts])
        self._check(self.lib.ampli_acc_merge(self.h, C.byref(dst.struct), arr, len(parts)))
        return dst

    def regions(self, P: int):
        """(sum_bytes, gm_offset, gm_bytes) of a table buffer (ampli_acc_regions)."""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.ampli_acc_regions(P, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def acc_pack(self, acc: Acc, packed):
        self._check(self.lib.ampli_acc_pack(self.h, C.byref(acc.struct), _ptr(packed)))

    def acc_unpack(self, packed, acc: Acc):
        self._check(self.lib.ampli_acc_unpack(self.h, _ptr(packed), C.byref(acc.struct)))

    def gm_merge(self, dst: Acc, regions, nparts: int):
        """regions: uint8 tensor holding nparts gathered gm regions back to back."""
        self._check(self.lib.ampli_gm_merge(self.h, C.byref(dst.struct), _ptr(regions), nparts))

    def error_finalize(self, acc: Acc, C_value: float = 0.002, cov: int = 100, out: ErrorTable | None = None) -> ErrorTable:
        import torch

        P = acc.P
        if out is None:
            out = self._new_error_table(P)
        self._check(self.lib.ampli_error_finalize(self.h, C.byref(acc.struct), C_value, cov, _ptr(out.rate), _ptr(out.code),
                                                  _ptr(out.thr), _ptr(out.germ_val), _ptr(out.germ_present), _ptr(out.flags)))
        return out

    def poisson_call(self, trecs, P: int, thr, ref_code, cov: int = 100, mode: int = POISSON_PREFILTER, E: int = 0,
                     ext_pos=None, call_mask=None, capacity: int = 0, dense_q: bool = False, dense_af: bool = False,
                     calls_buf=None, n_calls=None, blocks_of: int = 0, q=None, af=None):
        """thr: float32 [2, 4, P] thresholds -- or, with blocks_of = n > 0, the all-gathered blocks of an n-slice
        position-sliced merge (ampli_poisson_call_blocks: thresholds are read straight from the blocks).  q / af: the caller's own
        buffers for the dense scores (float64 [T, R, 4, 2]) and VAFs (float32 [T, R, 4, 3]) instead of dense_q / dense_af."""
        import torch

        assert trecs.dtype == self._rec_dtype() and trecs.is_cuda and trecs.is_contiguous()
        T = trecs.shape[0]
        R = P + E
        assert trecs.numel() == T * R * self._rec_elems()
        d = self.device
        if call_mask is None:
            call_mask = torch.empty(((T * R + 3) // 4 * 4,), dtype=torch.uint8, device=d)[: T * R].view(T, R)
        if q is None and dense_q:
            q = torch.empty((T, R, 4, 2), dtype=torch.float64, device=d)
        if af is None and dense_af:
            af = torch.empty((T, R, 4, 3), dtype=torch.float32, device=d)
        if capacity > 0 and calls_buf is None:
            calls_buf = torch.empty((capacity * C.sizeof(Call),), dtype=torch.uint8, device=d)
        if capacity > 0:
            capacity -= capacity % CALL_SHARDS
        if (capacity > 0 or n_calls is not None) and n_calls is None:
            n_calls = torch.zeros((CALL_COUNTER_WORDS,), dtype=torch.int64, device=d)
        if blocks_of > 0:
            self._check(self.lib.ampli_poisson_call_blocks(self.h, _ptr(trecs), P, E, _ptr(ext_pos), T, _ptr(thr), blocks_of,
                                                           _ptr(ref_code), cov, mode, _ptr(call_mask), _ptr(calls_buf), capacity,
                                                           _ptr(n_calls), _ptr(q), _ptr(af)))
        else:
            self._check(self.lib.ampli_poisson_call(self.h, _ptr(trecs), P, E, _ptr(ext_pos), T, _ptr(thr), _ptr(ref_code), cov,
                                                    mode, _ptr(call_mask), _ptr(calls_buf), capacity, _ptr(n_calls), _ptr(q), _ptr(af)))
        return dict(call_mask=call_mask, q=q, af=af, calls_buf=calls_buf, n_calls=n_calls, capacity=capacity)

    def _n_calls_total(self, res) -> int:
        """the entries of a compact call list (synchronises the context's stream; Context.n_calls_total(res) on the class: torch's current stream)"""
        read = (lambda self, res: int(res["n_calls"][::CALL_COUNTER_STRIDE].sum().item()))
        return read(None, res) if self is None else _on_stream(read)(self, res)

    n_calls_total = _StaticOrBound(_n_calls_total)

    def read_calls(self, res) -> list[dict]:
        """Copy the compact call list to the host, sorted into the reference's emission order."""
        return self._read_list(res, Call)

    def score_batch(self, k, rd, err):
        import torch

        n = k.numel()
        q = torch.empty(n, dtype=torch.float64, device=self.device)
        p = torch.empty(n, dtype=torch.float64, device=self.device)
        self._check(self.lib.ampli_score_batch(self.h, _ptr(k), _ptr(rd), _ptr(err), n, _ptr(q), _ptr(p)))
        return q, p

    def score_dense_batch(self, k, rd, err):
        """Q by the all-scores mode's scorer (ampli_poisson_score_dense)"""
        import torch

        q = torch.empty(k.numel(), dtype=torch.float64, device=self.device)
        self._check(self.lib.ampli_score_dense_batch(self.h, _ptr(k), _ptr(rd), _ptr(err), k.numel(), _ptr(q)))
        return q

    def drain_score_batch(self, k, rd, err):
        """(Q, p) by the scorer of the prefilter mode's drain (ampli_drain_p) for counts k above the mean rd * err > 0"""
        import torch

        n = k.numel()
        q = torch.empty(n, dtype=torch.float64, device=self.device)
        p = torch.empty(n, dtype=torch.float64, device=self.device)
        self._check(self.lib.ampli_drain_score_batch(self.h, _ptr(k), _ptr(rd), _ptr(err), n, _ptr(q), _ptr(p)))
        return q, p

    def roundtrip_batch(self, x):
        import torch

        out = torch.empty_like(x)
        self._check(self.lib.ampli_roundtrip_batch(self.h, _ptr(x), x.numel(), _ptr(out)))
        return out

    def synth_fill(self, P: int, n_samples: int, first_sample: int = 0, seed: int = 0xA3F15017, depth: int = 2000,
                   tumour: bool = False, out=None):
        import torch

        if out is None:
            out = torch.empty((n_samples, P, 8), dtype=torch.int32, device=self.device)
        self._check(self.lib.ampli_synth_fill(self.h, _ptr(out), P, n_samples, first_sample, seed, depth, int(tumour)))
        return out

    def synth_ref(self, P: int, seed: int = 0xA3F15017):
        import torch

        out = torch.empty((P,), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ampli_synth_ref(self.h, _ptr(out), P, seed))
        return out


# The stream contract in one place: every method that allocates, fills, uploads or reads back with torch runs under the context's
# stream.  Left as they are: what touches no tensor (setters, getters, events, graph handles, sync) and what only wraps pointers;
# n_calls_total places itself.  Plain functions only: anything else that is added to the class (a staticmethod, a property) has to be
# placed by hand, and says so here.
_PLAIN = {"close", "sync", "records", "dilution_records", "pack", "set_record_layout", "set_tuning", "last_reduce_kernel", "graph_begin", "graph_end",
          "graph_launch", "graph_destroy", "set_async_drain", "wait_calls", "set_ranges", "ranges_concurrent", "ranges_join", "range_record",
          "set_reduce_compact", "set_slice_format", "set_poisson_tuning", "set_queue_items", "flags", "event", "record", "elapsed_ms", "limit_stats",
          "power_stats", "last_spectrum_segments", "fdr_workspace_bytes", "set_slice_group", "slice_len", "regions"}
for _name, _fn in list(vars(Context).items()):
    if _name.startswith("__") or _name in ("LAYOUTS", "n_calls_total"):
        continue
    assert inspect.isfunction(_fn), f"Context.{_name} is no plain function: place it on the context's stream by hand"
    if _name not in _PLAIN and (not _name.startswith("_") or _name == "_read_list"):
        setattr(Context, _name, _on_stream(_fn))
del _name, _fn
