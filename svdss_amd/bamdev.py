"""BAM records walked, filtered and searched on the GPU: Python binding of svdss_bam_batch_run (csrc/bam_device.hip),
which stands where PingPong::load_batch_bam + process_batch stand (/root/reference/ping_pong.cpp:53-128,176-209).
The host side here does what the binary's scanner does: find the BGZF blocks, read the BAM header, cut the file into
batches of consecutive blocks."""
import ctypes as C
import struct
import zlib

import numpy as np

from . import bgzf
from ._lib import SVDSS_BAM_PUTATIVE, SVDSS_SFS_ASSEMBLE, SvdssError, lib


class BamResult(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_slots", C.c_int64), ("n_searched", C.c_int64), ("n_short", C.c_int64),
                ("total_sfs", C.c_int64), ("name_off", C.POINTER(C.c_int32)), ("names", C.POINTER(C.c_char)),
                ("hp", C.POINTER(C.c_int32)), ("sidx", C.POINTER(C.c_int32)), ("counts", C.POINTER(C.c_int64)),
                ("qs", C.POINTER(C.c_int32)), ("len", C.POINTER(C.c_int32)), ("inflate_kernel_ms", C.c_double),
                ("stage_ms", C.c_double * 8)]


def bam_header(data, blocks):
    """(n_ref, header bytes of the inflated stream) -- inflates leading blocks on the host until the header is complete."""
    buf = b""
    k = 0

    def need(n):
        nonlocal buf, k
        while len(buf) < n:
            if k >= len(blocks):
                raise ValueError("truncated header")
            coff, clen, isize, _ = blocks[k]
            buf += zlib.decompress(bytes(data[coff:coff + clen]), -15)
            k += 1
    need(12)
    if buf[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    l_text = struct.unpack_from("<i", buf, 4)[0]
    need(12 + l_text)
    n_ref = struct.unpack_from("<i", buf, 8 + l_text)[0]
    o = 12 + l_text
    for _ in range(n_ref):
        need(o + 4)
        l_name = struct.unpack_from("<i", buf, o)[0]
        o += 4 + l_name + 4
        need(o)
    return n_ref, o


def set_gate(stream, gate):
    """svdss_bam_stream_set_regions: `gate` = [(tid, beg, end)] sorted by (tid, beg) and merged, 0-based half open (an
    empty list: no record is in; None: no gate).  Before the stream's batch 0."""
    if gate is None:
        return
    t = np.array([g[0] for g in gate], dtype=np.int32)
    b = np.array([g[1] for g in gate], dtype=np.int32)
    e = np.array([g[2] for g in gate], dtype=np.int32)
    rc = lib.svdss_bam_stream_set_regions(stream, len(gate), t.ctypes.data if len(gate) else None, b.ctypes.data if len(gate) else None,
                                          e.ctypes.data if len(gate) else None)
    if rc:
        raise SvdssError(rc, "svdss_bam_stream_set_regions")


def search_bam(index, data, assemble=True, putative=False, batch_bytes=256 << 20, n_ref=None, skip=None, gate=None, chunks_per_batch=1):
    """`data`: the bytes of a BAM file.  Runs the whole file through svdss_bam_batch_run in batches of about
    batch_bytes inflated bytes (one after the other; the binary runs several at once) and returns a list of
    (name, hp, None | [(qs, len), ...]) for every record that passed the filters, in file order, plus a dict of counters.
    chunks_per_batch: every batch's members handed over as that many chunks (bgzf.BatchArgs.split)."""
    blocks = bgzf.bgzf_blocks(data)
    if n_ref is None or skip is None:
        n_ref, skip = bam_header(data, blocks)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    stream = C.c_void_p()
    rc = lib.svdss_bam_stream_create(n_ref, C.byref(stream))
    if rc:
        raise SvdssError(rc, "svdss_bam_stream_create")
    batch = C.c_void_p()
    out, stats = [], {"records": 0, "short": 0, "batches": 0}
    set_gate(stream, gate)
    flags = (SVDSS_SFS_ASSEMBLE if assemble else 0) | (SVDSS_BAM_PUTATIVE if putative else 0)
    try:
        groups = bgzf.batches(data, batch_bytes)   # (the last one possibly empty: it closes the stream)
        for seq, g in enumerate(groups):
            A = bgzf.BatchArgs.of(comp, g, chunks_per_batch)
            rc = lib.svdss_bam_batch_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, index._h, *A.args,
                                         flags, C.byref(batch))
            if rc:
                e = SvdssError(rc, "svdss_bam_batch_run")
                e.detail = (lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""
                if not e.detail:
                    e.detail = lib.svdss_bam_stream_error(stream).decode()
                raise e
            r = BamResult()
            lib.svdss_bam_batch_result(batch, C.byref(r))
            stats["records"] += r.n_records
            stats["short"] += r.n_short
            stats["batches"] += 1
            n = r.n_slots
            name_off = np.ctypeslib.as_array(r.name_off, shape=(n + 1,)).copy() if n else np.zeros(1, np.int32)
            names = C.string_at(r.names, int(name_off[-1])) if n else b""
            hp = np.ctypeslib.as_array(r.hp, shape=(n,)).copy() if n else np.zeros(0, np.int32)
            sidx = np.ctypeslib.as_array(r.sidx, shape=(n,)).copy() if n else np.zeros(0, np.int32)
            counts = np.ctypeslib.as_array(r.counts, shape=(r.n_searched,)).copy() if r.n_searched else np.zeros(0, np.int64)
            qs = np.ctypeslib.as_array(r.qs, shape=(r.total_sfs,)).copy() if r.total_sfs else np.zeros(0, np.int32)
            ln = np.ctypeslib.as_array(r.len, shape=(r.total_sfs,)).copy() if r.total_sfs else np.zeros(0, np.int32)
            first = np.concatenate([[0], np.cumsum(counts)])
            for i in range(n):
                nm = names[name_off[i]:name_off[i + 1]].decode()
                k = int(sidx[i])
                sfs = None if k < 0 else [(int(qs[j]), int(ln[j])) for j in range(int(first[k]), int(first[k + 1]))]
                out.append((nm, int(hp[i]), sfs))
        nseg = C.c_int64(0)
        stats["rewalked"] = lib.svdss_bam_stream_rewalked(stream, C.byref(nseg))
        stats["segments"] = nseg.value
        stats["gated"] = lib.svdss_bam_stream_gated(stream)
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        lib.svdss_bam_stream_free(stream)
    return out, stats


class BamSelection(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_selected", C.c_int64), ("n_bytes", C.c_int64), ("rec_off", C.POINTER(C.c_int64)),
                ("bytes", C.POINTER(C.c_uint8)), ("inflate_kernel_ms", C.c_double), ("stage_ms", C.c_double * 8),
                ("slim", C.c_int32)]


class BamInputFrag(C.Structure):
    _fields_ = [("on", C.c_int32), ("unsorted", C.c_int32), ("n_records", C.c_int64), ("n_no_coor", C.c_int64), ("n_chunks", C.c_int64),
                ("chunks", C.c_void_p), ("n_windows", C.c_int64), ("windows", C.c_void_p), ("first_tid", C.c_int32), ("last_tid", C.c_int32),
                ("first_beg", C.c_int64), ("last_beg", C.c_int64), ("comp_bytes", C.c_int64), ("first_data", C.c_int64),
                ("ends_at_boundary", C.c_int32)]


def set_input_index(stream, scheme):
    """svdss_bam_stream_set_input_index: `scheme` = (min_shift, depth), None: the switch stays off.  Before the stream's batch 0."""
    if scheme is None:
        return
    rc = lib.svdss_bam_stream_set_input_index(stream, int(scheme[0]), int(scheme[1]))
    if rc:
        raise SvdssError(rc, "svdss_bam_stream_set_input_index")


def bam_ref_lengths(data, blocks):
    """the reference lengths of the BAM header, in order"""
    n_ref, skip = bam_header(data, blocks)
    buf = b""
    for coff, clen, isize, _ in blocks:
        buf += zlib.decompress(bytes(data[coff:coff + clen]), -15)
        if len(buf) >= skip:
            break
    o = 12 + struct.unpack_from("<i", buf, 4)[0]
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", buf, o)[0]
        lens.append(struct.unpack_from("<i", buf, o + 4 + l_name)[0])
        o += 8 + l_name
    return lens


def index_bam(data, csi=False, batch_bytes=256 << 20, device=0, chunks_per_batch=1):
    """The BAI (csi=True: CSI) index of a BAM file (bytes), built on the GPU: select_bam's loop with the stream's input index
    switched on (svdss_bam_stream_set_input_index) and every batch's fragments folded in file order
    (svdss_bam_input_indexer_*).  The bytes `SVDSS bamindex` writes.  SvdssError with code SVDSS_EIO for an unsorted file."""
    blocks = bgzf.bgzf_blocks(data)
    lens = np.array(bam_ref_lengths(data, blocks), dtype=np.int32)
    ix, shift, depth = C.c_void_p(), C.c_int32(0), C.c_int32(0)
    rc = lib.svdss_bam_input_indexer_create(len(lens), lens.ctypes.data if len(lens) else None, 1 if csi else 0, C.byref(shift), C.byref(depth),
                                            C.byref(ix))
    if rc:
        raise SvdssError(rc, "svdss_bam_input_indexer_create")
    try:
        base = 0

        def fold(batch):
            nonlocal base
            f = BamInputFrag()
            _check(lib.svdss_bam_batch_input_index(batch, C.byref(f)), "svdss_bam_batch_input_index")
            _check(lib.svdss_bam_input_indexer_add(ix, C.byref(f), base), "svdss_bam_input_indexer_add")
            base += f.comp_bytes
        select_bam(data, names=[], batch_bytes=batch_bytes, device=device, input_index=(shift.value, depth.value), on_batch=fold,
                   chunks_per_batch=chunks_per_batch)
        # the end of the stream: the EOF marker where the file ends with one, else the file's size
        end = len(data)
        if blocks and blocks[-1][2] == 0:
            end = blocks[-1][0] - 18
        out, n = C.c_void_p(), C.c_int64(0)
        _check(lib.svdss_bam_input_indexer_finish(ix, end, C.byref(out), C.byref(n)), "svdss_bam_input_indexer_finish")
        return C.string_at(out, n.value)
    finally:
        lib.svdss_bam_input_indexer_free(ix)


def select_bam(data, names=None, regions=None, min_mapq=0, batch_bytes=256 << 20, device=0, gate=None, input_index=None, on_batch=None,
               chunks_per_batch=1):
    """svdss_bam_select_run over a whole BAM file (bytes): the records `SVDSS call` keeps -- no flag 4 / 256 / 2048,
    mapq >= min_mapq, and (when given) read name in `names` or alignment overlapping one of `regions` =
    [(tid, beg, end)] sorted by (tid, beg).  Returns ([record bytes without the block_size field], counters).
    input_index: see set_input_index; on_batch(batch handle): called after every batch; chunks_per_batch: every batch's
    members handed over as that many chunks (bgzf.BatchArgs.split)."""
    blocks = bgzf.bgzf_blocks(data)
    n_ref, skip = bam_header(data, blocks)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    nm = b"".join(n.encode() if isinstance(n, str) else n for n in (names or []))
    nm_off = np.zeros(len(names or []) + 1, dtype=np.int64)
    if names:
        nm_off[1:] = np.cumsum([len(n) for n in names])
    rt = np.array([r[0] for r in (regions or [])], dtype=np.int32)
    rb = np.array([r[1] for r in (regions or [])], dtype=np.int32)
    re_ = np.array([r[2] for r in (regions or [])], dtype=np.int32)
    flt = C.c_void_p()
    rc = lib.svdss_bam_filter_create(device, min_mapq, n_ref, nm if names else None, nm_off.ctypes.data if names else None, len(names or []),
                                     rt.ctypes.data if regions else None, rb.ctypes.data if regions else None,
                                     re_.ctypes.data if regions else None, len(regions or []), C.byref(flt))
    if rc:
        raise SvdssError(rc, "svdss_bam_filter_create")
    stream = C.c_void_p()
    lib.svdss_bam_stream_create(n_ref, C.byref(stream))
    batch = C.c_void_p()
    out, stats = [], {"records": 0, "batches": 0}
    try:
        set_gate(stream, gate)
        set_input_index(stream, input_index)
        groups = bgzf.batches(data, batch_bytes)
        for seq, g in enumerate(groups):
            A = bgzf.BatchArgs.of(comp, g, chunks_per_batch)
            rc = lib.svdss_bam_select_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, flt, *A.args, C.byref(batch))
            if rc:
                e = SvdssError(rc, "svdss_bam_select_run")
                e.detail = (lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""
                raise e
            r = BamSelection()
            lib.svdss_bam_batch_selection(batch, C.byref(r))
            stats["records"] += r.n_records
            stats["batches"] += 1
            if on_batch is not None:
                on_batch(batch)
            if r.n_selected:
                off = np.ctypeslib.as_array(r.rec_off, shape=(r.n_selected + 1,))
                raw = C.string_at(r.bytes, r.n_bytes)
                for k in range(r.n_selected):
                    o = int(off[k])
                    bs = struct.unpack_from("<i", raw, o)[0]
                    out.append(raw[o + 4:o + 4 + bs])
        stats["gated"] = lib.svdss_bam_stream_gated(stream)
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        lib.svdss_bam_stream_free(stream)
        lib.svdss_bam_filter_free(flt)
    return out, stats


SVDSS_BAM_SKIP_RESTART = 1 << 40


def select_bam_ranges(data, ranges, min_mapq=0, batch_blocks=16, device=0, gate=None):
    """svdss_bam_select_run over RANGES of a BAM file as one stream, the way `--region` with an index reads it: `ranges` =
    [(first block, end block, skip)] over bgzf.bgzf_blocks(data), ascending and disjoint, a record starting `skip` bytes into
    each range's first block (the first range may be (0, n, header length)).  Every range is cut into batches of
    batch_blocks blocks; the first batch of every range but the first carries SVDSS_BAM_SKIP_RESTART.  Returns the kept
    records' bytes (without the block_size field), in order."""
    blocks = bgzf.bgzf_blocks(data)
    n_ref, _ = bam_header(data, blocks)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    flt, stream, batch = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib.svdss_bam_filter_create(device, min_mapq, n_ref, None, None, 0, None, None, None, 0, C.byref(flt)), "svdss_bam_filter_create")
    _check(lib.svdss_bam_stream_create(n_ref, C.byref(stream)), "svdss_bam_stream_create")
    out = []
    try:
        _check(lib.svdss_bam_stream_region(stream, 0, 1, None, 0), "svdss_bam_stream_region")
        set_gate(stream, gate)
        jobs = []
        for k, (b0, b1, skip) in enumerate(ranges):
            for at in range(b0, b1, batch_blocks):
                jobs.append((blocks[at:min(at + batch_blocks, b1)], (skip | (SVDSS_BAM_SKIP_RESTART if k else 0)) if at == b0 else 0))
        if not jobs:
            jobs = [([], 0)]
        for seq, (g, skip) in enumerate(jobs):
            A = bgzf.BatchArgs.whole(comp, g)
            rc = lib.svdss_bam_select_run(stream, seq, 1 if seq == len(jobs) - 1 else 0, skip, flt, *A.args, C.byref(batch))
            if rc:
                raise SvdssError(rc, "svdss_bam_select_run: " + ((lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""))
            r = BamSelection()
            lib.svdss_bam_batch_selection(batch, C.byref(r))
            if r.n_selected:
                off = np.ctypeslib.as_array(r.rec_off, shape=(r.n_selected + 1,))
                raw = C.string_at(r.bytes, r.n_bytes)
                for i in range(r.n_selected):
                    o = int(off[i])
                    out.append(raw[o + 4:o + 4 + struct.unpack_from("<i", raw, o)[0]])
        return out
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        lib.svdss_bam_stream_free(stream)
        lib.svdss_bam_filter_free(flt)


def select_bam_store(data, names, regions, min_mapq=0, batch_bytes=256 << 20, device=0, max_store_bytes=1 << 34, gate=None):
    """`SVDSS call`'s ONE pass: svdss_bam_select_store_run over a whole BAM file with `names` as the filter (the first pass'
    records come back whole) and every record that passes the flag / mapq filters kept, slim, in a svdss_bam_store_t; then
    svdss_bam_store_select of every stored batch with `regions` [(tid, beg, end)] sorted by (tid, beg).
    Returns (named records, slim records that overlap a region -- both without the block_size field --, counters)."""
    blocks = bgzf.bgzf_blocks(data)
    n_ref, skip = bam_header(data, blocks)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    nm = b"".join(n.encode() if isinstance(n, str) else n for n in names)
    nm_off = np.zeros(len(names) + 1, dtype=np.int64)
    nm_off[1:] = np.cumsum([len(n) for n in names])
    rt = np.array([r[0] for r in regions], dtype=np.int32)
    rb = np.array([r[1] for r in regions], dtype=np.int32)
    re_ = np.array([r[2] for r in regions], dtype=np.int32)
    f_names, f_regions, store = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.svdss_bam_filter_create(device, min_mapq, n_ref, nm, nm_off.ctypes.data, len(names), None, None, None, 0, C.byref(f_names))
    if rc:
        raise SvdssError(rc, "svdss_bam_filter_create")
    rc = lib.svdss_bam_filter_create(device, min_mapq, n_ref, None, None, 0, rt.ctypes.data if regions else None, rb.ctypes.data if regions else None,
                                     re_.ctypes.data if regions else None, len(regions), C.byref(f_regions))
    if rc:
        raise SvdssError(rc, "svdss_bam_filter_create")
    rc = lib.svdss_bam_store_create(device, max_store_bytes, min(max_store_bytes, 1 << 20), C.byref(store))
    if rc:
        raise SvdssError(rc, "svdss_bam_store_create")
    stream = C.c_void_p()
    lib.svdss_bam_stream_create(n_ref, C.byref(stream))
    batch = C.c_void_p()
    named, slim, stats = [], [], {"records": 0, "batches": 0}

    def take(r, into):
        if r.n_selected:
            off = np.ctypeslib.as_array(r.rec_off, shape=(r.n_selected + 1,))
            raw = C.string_at(r.bytes, r.n_bytes)
            for k in range(r.n_selected):
                o = int(off[k])
                bs = struct.unpack_from("<i", raw, o)[0]
                into.append(raw[o + 4:o + 4 + bs])
    try:
        set_gate(stream, gate)
        groups = bgzf.batches(data, batch_bytes)
        for seq, g in enumerate(groups):
            A = bgzf.BatchArgs.whole(comp, g)
            rc = lib.svdss_bam_select_store_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, f_names, store, *A.args,
                                                C.byref(batch))
            if rc:
                e = SvdssError(rc, "svdss_bam_select_store_run")
                e.detail = (lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""
                raise e
            r = BamSelection()
            lib.svdss_bam_batch_selection(batch, C.byref(r))
            # (with a store the first pass' records are slim too; once it is over its limit the batches behind come whole)
            stats["records"] += r.n_records
            stats["batches"] += 1
            stats.setdefault("named_slim", []).extend([int(r.slim)] * int(r.n_selected))
            take(r, named)
        stats["gated"] = lib.svdss_bam_stream_gated(stream)
        complete, n_rec, n_bytes = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        n_b = lib.svdss_bam_store_batches(store, C.byref(complete), C.byref(n_rec), C.byref(n_bytes))
        stats.update({"stored_batches": n_b, "complete": complete.value, "stored_records": n_rec.value, "stored_bytes": n_bytes.value})
        if complete.value:
            for seq in range(n_b):
                rc = lib.svdss_bam_store_select(store, seq, f_regions, C.byref(batch))
                if rc:
                    raise SvdssError(rc, "svdss_bam_store_select")
                r = BamSelection()
                lib.svdss_bam_batch_selection(batch, C.byref(r))
                assert r.slim == 1
                take(r, slim)
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        lib.svdss_bam_stream_free(stream)
        lib.svdss_bam_filter_free(f_names)
        lib.svdss_bam_filter_free(f_regions)
        lib.svdss_bam_store_free(store)
    return named, slim, stats


# ---- the record store filled by either route, and selections from it (`SVDSS run`: csrc/run_host.cpp)
class BamSmoothed(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_kept", C.c_int64), ("match_mismatch", C.POINTER(C.c_int64)), ("fits", C.POINTER(C.c_uint8)),
                ("out_bytes", C.c_int64), ("bgzf", C.POINTER(C.c_uint8)), ("bgzf_bytes", C.c_int64), ("n_xf", C.c_int64 * 4),
                ("inflate_kernel_ms", C.c_double), ("stage_ms", C.c_double * 8)]


def _check(rc, what):
    if rc:
        raise SvdssError(rc, what)


class BamFilter:
    """svdss_bam_filter_t: read names (a list, possibly empty; None: no name test) and / or regions [(tid, beg, end)] sorted
    by (tid, beg).  A record passes if its name's hash is in the set or its alignment overlaps a region."""

    def __init__(self, n_ref, names=None, regions=None, min_mapq=0, device=0):
        self._h = C.c_void_p()
        names = None if names is None else [n.encode() if isinstance(n, str) else n for n in names]
        nm = b"".join(names) if names is not None else None
        nm_off = np.zeros(len(names or []) + 1, dtype=np.int64)
        if names:
            nm_off[1:] = np.cumsum([len(n) for n in names])
        rt = np.array([r[0] for r in (regions or [])], dtype=np.int32)
        rb = np.array([r[1] for r in (regions or [])], dtype=np.int32)
        re_ = np.array([r[2] for r in (regions or [])], dtype=np.int32)
        _check(lib.svdss_bam_filter_create(device, min_mapq, n_ref, nm, nm_off.ctypes.data if names is not None else None, len(names or []),
                                           rt.ctypes.data if regions else None, rb.ctypes.data if regions else None,
                                           re_.ctypes.data if regions else None, len(regions or []), C.byref(self._h)), "svdss_bam_filter_create")

    def close(self):
        if self._h:
            lib.svdss_bam_filter_free(self._h)
            self._h = C.c_void_p()


class BamStore:
    """svdss_bam_store_t: the slim records of every batch, in HBM.  fill_by_select: svdss_bam_select_store_run (what `SVDSS
    call`'s first pass does); fill_by_smooth: svdss_bam_smooth_run after svdss_bam_smooth_set_store (what `SVDSS run` does).
    Both take the bytes of a BAM file and cut it into the same batches."""

    def __init__(self, max_bytes=1 << 34, initial_bytes=1 << 20, device=0):
        self._h = C.c_void_p()
        self.device = device
        _check(lib.svdss_bam_store_create(device, max_bytes, min(max_bytes, initial_bytes), C.byref(self._h)), "svdss_bam_store_create")

    def close(self):
        if self._h:
            lib.svdss_bam_store_free(self._h)
            self._h = C.c_void_p()

    def batches(self):
        """(stored batches, complete, records, bytes)"""
        complete, n_rec, n_bytes = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        n_b = lib.svdss_bam_store_batches(self._h, C.byref(complete), C.byref(n_rec), C.byref(n_bytes))
        return n_b, bool(complete.value), n_rec.value, n_bytes.value

    def select(self, seq, flt):
        """svdss_bam_store_select of stored batch `seq`: (the kept slim records' bytes, their n + 1 offsets)"""
        batch = C.c_void_p()
        try:
            _check(lib.svdss_bam_store_select(self._h, seq, flt._h, C.byref(batch)), "svdss_bam_store_select")
            r = BamSelection()
            lib.svdss_bam_batch_selection(batch, C.byref(r))
            assert r.slim == 1
            off = np.ctypeslib.as_array(r.rec_off, shape=(r.n_selected + 1,)).copy()
            return (C.string_at(r.bytes, r.n_bytes) if r.n_bytes else b""), off
        finally:
            if batch:
                lib.svdss_bam_batch_free(batch)

    def fill_by_select(self, data, min_mapq=0, batch_bytes=256 << 20, gate=None):
        """every batch of the file through svdss_bam_select_store_run with an empty set of names; returns the batch count"""
        blocks = bgzf.bgzf_blocks(data)
        n_ref, skip = bam_header(data, blocks)
        comp = np.frombuffer(bytes(data), dtype=np.uint8)
        flt = BamFilter(n_ref, names=[], min_mapq=min_mapq, device=self.device)
        stream, batch = C.c_void_p(), C.c_void_p()
        _check(lib.svdss_bam_stream_create(n_ref, C.byref(stream)), "svdss_bam_stream_create")
        try:
            set_gate(stream, gate)
            groups = bgzf.batches(data, batch_bytes)
            for seq, g in enumerate(groups):
                A = bgzf.BatchArgs.whole(comp, g)
                rc = lib.svdss_bam_select_store_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, flt._h, self._h, *A.args,
                                                    C.byref(batch))
                if rc:
                    raise SvdssError(rc, "svdss_bam_select_store_run: " + ((lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""))
            return len(groups)
        finally:
            if batch:
                lib.svdss_bam_batch_free(batch)
            lib.svdss_bam_stream_free(stream)
            flt.close()


def smooth_bam(data, contigs_ascii, min_mapq=20, acc=1.0, batch_bytes=256 << 20, store=None, store_min_mapq=None, device=0, gate=None,
               measure=False, input_index=None):
    """svdss_bam_smooth_run over a whole BAM file (bytes) whose header names `contigs_ascii` in order; with `store` (a
    BamStore) after svdss_bam_smooth_set_store(sm, store, store_min_mapq).  Returns (the BGZF members of the smoothed
    stream, batch count).  gate: see set_gate.  measure=True: svdss_bam_smooth_measure instead -- returns ([(matches,
    mismatches, fits) per kept record, in file order], [(n_records, n_kept) per batch]).  input_index: see set_input_index."""
    blocks = bgzf.bgzf_blocks(data)
    n_ref, skip = bam_header(data, blocks)
    raw_head = b""
    for coff, clen, isize, _ in blocks:
        raw_head += zlib.decompress(bytes(data[coff:coff + clen]), -15)
        if len(raw_head) >= skip:
            break
    resident = contigs_ascii if hasattr(contigs_ascii, "_h") else None   # (refdev.ResidentRef: the chromosomes are in HBM already)
    n_contigs = resident.n if resident else len(contigs_ascii)
    tid_map = np.full(n_ref, -1, dtype=np.int32)
    tid_map[:n_contigs] = np.arange(n_contigs, dtype=np.int32)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    ref, sm, stream, batch = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    out = bytearray()
    try:
        if resident is None:
            cat = np.frombuffer("".join(contigs_ascii).encode(), dtype=np.uint8)
            off = np.concatenate([[0], np.cumsum([len(c) for c in contigs_ascii])]).astype(np.int64)
            _check(lib.svdss_ref_upload(cat.ctypes.data, off.ctypes.data, len(contigs_ascii), device, C.byref(ref)), "svdss_ref_upload")
        _check(lib.svdss_bam_smooth_create(resident._h if resident else ref, tid_map.ctypes.data, n_ref, min_mapq, C.byref(sm)), "svdss_bam_smooth_create")
        if store is not None:
            _check(lib.svdss_bam_smooth_set_store(sm, store._h, min_mapq if store_min_mapq is None else store_min_mapq), "svdss_bam_smooth_set_store")
        _check(lib.svdss_bam_stream_create(n_ref, C.byref(stream)), "svdss_bam_stream_create")
        head = np.frombuffer(raw_head[:skip], dtype=np.uint8)
        _check(lib.svdss_bam_stream_set_output_prefix(stream, head.ctypes.data, len(head)), "svdss_bam_stream_set_output_prefix")
        set_gate(stream, gate)
        set_input_index(stream, input_index)
        groups = bgzf.batches(data, batch_bytes)
        measured, counts = [], []
        for seq, g in enumerate(groups):
            A = bgzf.BatchArgs.whole(comp, g)
            if measure:
                rc = lib.svdss_bam_smooth_measure(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, sm, *A.args, C.byref(batch))
                if rc:
                    raise SvdssError(rc, "svdss_bam_smooth_measure: " + ((lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""))
                sr = BamSmoothed()
                _check(lib.svdss_bam_batch_smoothed(batch, C.byref(sr)), "svdss_bam_batch_smoothed")
                counts.append((int(sr.n_records), int(sr.n_kept)))
                for k in range(sr.n_kept):
                    measured.append((int(sr.match_mismatch[2 * k]), int(sr.match_mismatch[2 * k + 1]), int(sr.fits[k])))
                continue
            rc = lib.svdss_bam_smooth_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, sm, C.c_double(acc), None, 0,
                                          *A.args, C.byref(batch))
            if rc:
                raise SvdssError(rc, "svdss_bam_smooth_run: " + ((lib.svdss_bam_batch_error(batch) or b"").decode() if batch else ""))
            sr = BamSmoothed()
            _check(lib.svdss_bam_batch_smoothed(batch, C.byref(sr)), "svdss_bam_batch_smoothed")
            out += C.string_at(sr.bgzf, sr.bgzf_bytes) if sr.bgzf_bytes else b""
        if measure:
            return measured, counts
        return bytes(out), len(groups)
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        if stream:
            lib.svdss_bam_stream_free(stream)
        if sm:
            lib.svdss_bam_smooth_free(sm)
        if ref:
            lib.svdss_ref_free(ref)
