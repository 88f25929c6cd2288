"""FASTA / FASTQ records found on the GPU: Python binding of svdss_fastx_batch_run (csrc/fastx_device.hip), which stands
where the kseq loop of PingPong::load_batch_fastq stands (/root/reference/ping_pong.cpp:130-173).  The host side here does
what the binary's batcher does (csrc/fastx_device.h): cut the input into batches -- runs of consecutive BGZF members, or
slices of plain text -- and hand them over in file order."""
import ctypes as C

import numpy as np

from . import bgzf as _bgzf
from ._lib import SVDSS_SFS_ASSEMBLE, SvdssError, lib


class FastxResult(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("name_off", C.POINTER(C.c_int32)), ("names", C.POINTER(C.c_char)),
                ("seq_len", C.POINTER(C.c_int32)), ("counts", C.POINTER(C.c_int64)), ("qs", C.POINTER(C.c_int32)),
                ("len", C.POINTER(C.c_int32)), ("total_sfs", C.c_int64), ("reads", C.POINTER(C.c_uint8)),
                ("offsets", C.POINTER(C.c_int64)), ("declined", C.c_int32), ("n_text_bytes", C.c_int64),
                ("text", C.POINTER(C.c_uint8)), ("text_bytes", C.c_int64), ("inflate_kernel_ms", C.c_double),
                ("parse_kernel_ms", C.c_double), ("stage_ms", C.c_double * 8)]


def tile_bytes():
    return int(lib.svdss_fastx_tile_bytes())


def plain_batches(data, batch_bytes):
    """(offset, length) of the slices of plain text; the last one closes the stream (an empty input has one empty batch)."""
    out, off = [], 0
    while True:
        n = min(batch_bytes, len(data) - off)
        out.append((off, n))
        off += n
        if off >= len(data):
            return out


def _run(data, batch_bytes, bgzf, carry_cap, index, assemble, device, chunks_per_batch=1):
    data = bytes(data)
    comp = np.frombuffer(data, dtype=np.uint8)
    stream = C.c_void_p()
    rc = lib.svdss_fastx_stream_create(device, batch_bytes if carry_cap is None else carry_cap, C.byref(stream))
    if rc:
        raise SvdssError(rc, "svdss_fastx_stream_create")
    batch = C.c_void_p()
    names, flat, lens, sfs, rest = [], [], [], [], []
    declined_at = None
    stats = {"batches": 0, "device_batches": 0, "host_batches": 0, "parse_ms": 0.0, "inflate_ms": 0.0, "text_bytes": 0}
    flags = SVDSS_SFS_ASSEMBLE if assemble else 0
    jobs = _bgzf.batches(data, batch_bytes) if bgzf else plain_batches(data, batch_bytes)
    try:
        for seq, g in enumerate(jobs):
            last = 1 if seq == len(jobs) - 1 else 0
            ix = index._h if index is not None else None
            if bgzf:
                A = _bgzf.BatchArgs.of(comp, g, chunks_per_batch)
                rc = lib.svdss_fastx_batch_run(stream, seq, last, ix, *A.args, None, 0, flags, C.byref(batch))
            else:
                rc = lib.svdss_fastx_batch_run(stream, seq, last, ix, 0, None, None, None, None, None,
                                               comp.ctypes.data + g[0] if g[1] else None, g[1], flags, C.byref(batch))
            if rc:
                e = SvdssError(rc, "svdss_fastx_batch_run")
                e.detail = (lib.svdss_fastx_batch_error(batch) or b"").decode() if batch else ""
                if not e.detail:
                    e.detail = lib.svdss_fastx_stream_error(stream).decode()
                raise e
            r = FastxResult()
            lib.svdss_fastx_batch_result(batch, C.byref(r))
            stats["batches"] += 1
            stats["parse_ms"] += r.parse_kernel_ms
            stats["inflate_ms"] += r.inflate_kernel_ms
            n = r.n_records
            if n:
                name_off = np.ctypeslib.as_array(r.name_off, shape=(n + 1,))
                raw = C.string_at(r.names, int(name_off[-1]))
                names += [raw[name_off[i]:name_off[i + 1]] for i in range(n)]
                lens.append(np.ctypeslib.as_array(r.seq_len, shape=(n,)).copy())
                if index is None:
                    off = np.ctypeslib.as_array(r.offsets, shape=(n + 1,))
                    assert (np.diff(off) == lens[-1]).all()
                    if off[-1]:
                        flat.append(np.ctypeslib.as_array(r.reads, shape=(int(off[-1]),)).copy())
                else:
                    counts = np.ctypeslib.as_array(r.counts, shape=(n,))
                    qs = np.ctypeslib.as_array(r.qs, shape=(r.total_sfs,)) if r.total_sfs else np.zeros(0, np.int32)
                    ln = np.ctypeslib.as_array(r.len, shape=(r.total_sfs,)) if r.total_sfs else np.zeros(0, np.int32)
                    first = np.concatenate([[0], np.cumsum(counts)])
                    sfs += [[(int(qs[j]), int(ln[j])) for j in range(int(first[i]), int(first[i + 1]))] for i in range(n)]
            if r.declined:
                if declined_at is None:
                    declined_at = seq
                stats["host_batches"] += 1
                rest.append(C.string_at(r.text, r.text_bytes))
            else:
                stats["device_batches"] += 1
                stats["text_bytes"] += r.n_text_bytes
    finally:
        if batch:
            lib.svdss_fastx_batch_free(batch)
        lib.svdss_fastx_stream_free(stream)
    stats["rest"] = b"".join(rest)
    lens = np.concatenate(lens) if lens else np.zeros(0, np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
    return names, (np.concatenate(flat) if flat else np.zeros(0, np.uint8)), offsets, declined_at, stats, sfs


def parse_fastx(data, batch_bytes, bgzf=False, carry_cap=None, device=0, chunks_per_batch=1):
    """`data`: the bytes of a FASTA / FASTQ file, plain or (bgzf=True) as BGZF members.  Parses it on the GPU in batches of
    batch_bytes and returns (names, nt6 symbols of all reads back to back, int64 offsets, the batch that declined or None,
    counters).  Records behind a declined batch are not delivered: counters["rest"] is the text from the first unparsed
    byte on, which the caller reads with the host reader.  chunks_per_batch: every batch's members handed over as that many
    chunks (bgzf.BatchArgs.split)."""
    return _run(data, batch_bytes, bgzf, carry_cap, None, True, device, chunks_per_batch)[:5]


def search_fastx(index, data, batch_bytes=192 << 20, bgzf=False, assemble=True, carry_cap=None):
    """parse_fastx followed by the search on `index` (resident on a device): (names, offsets, SFS per record as
    [(qs, len), ...], the batch that declined or None, counters)."""
    names, _, offsets, declined_at, stats, sfs = _run(data, batch_bytes, bgzf, carry_cap, index, assemble, 0)
    return names, offsets, sfs, declined_at, stats
