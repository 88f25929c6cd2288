"""The reference FASTA inflated and parsed on the GPU: Python binding of svdss_ref_stream_* (csrc/ref_stream.hip), which
stands where load_chromosomes stands on the host (csrc/fastx_reader.h).  The host side here does what the binary's loader
does (csrc/ref_loader.h): cut the input into batches -- runs of consecutive BGZF members, or slices of plain text -- and
hand them over in file order."""
import ctypes as C

import numpy as np

from . import bgzf as _bgzf
from ._lib import SvdssError, lib
from .fastxdev import plain_batches

DEFAULT_HEADER_CAP = 64 << 10
REASONS = {1: "cr", 2: "nul", 3: "at-line", 4: "not-fasta", 5: "duplicate-name", 6: "long-header", 7: "empty", 8: "io", 9: "error"}


class RefStreamResult(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("name_off", C.POINTER(C.c_int64)), ("names", C.POINTER(C.c_char)),
                ("seq_off", C.POINTER(C.c_int64)), ("declined", C.c_int32), ("declined_at", C.c_int64),
                ("n_batches", C.c_int64), ("text_bytes", C.c_int64), ("inflate_kernel_ms", C.c_double),
                ("parse_kernel_ms", C.c_double)]


def tile_bytes():
    return int(lib.svdss_ref_stream_tile_bytes())


class RefStream:
    """One FASTA read through svdss_ref_stream_batch: names, seq_off, declined (a key of REASONS or None), counters."""

    def __init__(self, data, batch_bytes, bgzf=False, header_cap=None, device=0, jobs=None, chunks_per_batch=1):
        data = bytes(data)
        comp = np.frombuffer(data, dtype=np.uint8)
        self._h = C.c_void_p()
        self.device = device
        rc = lib.svdss_ref_stream_create(device, DEFAULT_HEADER_CAP if header_cap is None else header_cap, C.byref(self._h))
        if rc:
            raise SvdssError(rc, "svdss_ref_stream_create")
        if jobs is None:
            jobs = _bgzf.batches(data, batch_bytes) if bgzf else plain_batches(data, batch_bytes)
        try:
            for seq, g in enumerate(jobs):
                last = 1 if seq == len(jobs) - 1 else 0
                if bgzf:
                    A = _bgzf.BatchArgs.of(comp, g, chunks_per_batch)
                    rc = lib.svdss_ref_stream_batch(self._h, seq, last, *A.args, None, 0)
                else:
                    rc = lib.svdss_ref_stream_batch(self._h, seq, last, 0, None, None, None, None, None,
                                                    comp.ctypes.data + g[0] if g[1] else None, g[1])
                if rc:
                    e = SvdssError(rc, "svdss_ref_stream_batch")
                    e.detail = lib.svdss_ref_stream_error(self._h).decode()
                    e.reason = self._result().declined
                    raise e
            r = self._result()
            self.declined = REASONS[r.declined] if r.declined else None
            self.declined_at = int(r.declined_at)
            self.detail = lib.svdss_ref_stream_error(self._h).decode()
            self.counters = {"batches": int(r.n_batches), "text_bytes": int(r.text_bytes), "inflate_ms": r.inflate_kernel_ms,
                             "parse_ms": r.parse_kernel_ms, "declined_at": self.declined_at}
            n = int(r.n_records)
            self.names, self.seq_off = [], np.zeros(1, np.int64)
            if n:
                name_off = np.ctypeslib.as_array(r.name_off, shape=(n + 1,))
                raw = C.string_at(r.names, int(name_off[-1]))
                self.names = [raw[name_off[i]:name_off[i + 1]] for i in range(n)]
                self.seq_off = np.ctypeslib.as_array(r.seq_off, shape=(n + 1,)).copy()
        except BaseException:
            self.close()
            raise

    def _result(self):
        r = RefStreamResult()
        lib.svdss_ref_stream_result(self._h, C.byref(r))
        return r

    def download(self, rec):
        n = int(self.seq_off[rec + 1] - self.seq_off[rec])
        dst = np.zeros(max(1, n), np.uint8)
        rc = lib.svdss_ref_stream_download(self._h, rec, dst.ctypes.data)
        if rc:
            raise SvdssError(rc, "svdss_ref_stream_download")
        return dst[:n].tobytes()

    def finish(self, order):
        order = np.ascontiguousarray(order, dtype=np.int32)
        ref = C.c_void_p()
        rc = lib.svdss_ref_stream_finish(self._h, order.ctypes.data if len(order) else None, len(order), self.device, C.byref(ref))
        if rc:
            raise SvdssError(rc, "svdss_ref_stream_finish")
        return ResidentRef(ref, len(order))

    def close(self):
        if self._h:
            lib.svdss_ref_stream_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ResidentRef:
    """A svdss_ref_t in HBM (what svdss_ref_upload builds); bamdev.smooth_bam takes one in place of the contigs."""

    def __init__(self, handle, n):
        self._h, self.n = handle, n

    def read(self):
        """(offsets, the chromosomes back to back) as they stand on the device."""
        off = np.zeros(self.n + 1, np.int64)
        n = C.c_int32()
        rc = lib.svdss_ref_read(self._h, C.byref(n), off.ctypes.data, None)
        if rc:
            raise SvdssError(rc, "svdss_ref_read")
        seqs = np.zeros(max(1, int(off[-1])), np.uint8)
        rc = lib.svdss_ref_read(self._h, C.byref(n), off.ctypes.data, seqs.ctypes.data)
        if rc:
            raise SvdssError(rc, "svdss_ref_read")
        assert n.value == self.n
        return off, seqs[:int(off[-1])].tobytes()

    def close(self):
        if self._h:
            lib.svdss_ref_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load_reference(data, batch_bytes, bgzf=False, header_cap=None, device=0, jobs=None, chunks_per_batch=1):
    """`data`: the bytes of a FASTA file, plain or (bgzf=True) as BGZF members.  Reads it on the GPU in batches of
    batch_bytes and returns (names, [upper-cased bytes per record], why it declined or None, counters).  A declined file
    delivers nothing: the caller reads it with the host reader."""
    with RefStream(data, batch_bytes, bgzf, header_cap, device, jobs, chunks_per_batch) as s:
        if s.declined:
            return [], [], s.declined, s.counters
        return s.names, [s.download(i) for i in range(len(s.names))], None, s.counters


def resident(data, batch_bytes, order=None, bgzf=False, header_cap=None, device=0):
    """The records of `data` (all of them in file order, or those `order` lists) as a ResidentRef on `device`, built by
    svdss_ref_stream_finish; raises ValueError with the reason if the stream declined."""
    with RefStream(data, batch_bytes, bgzf, header_cap, device) as s:
        if s.declined:
            raise ValueError(f"reference declined: {s.declined} at byte {s.declined_at}")
        return s.finish(np.arange(len(s.names)) if order is None else order)
