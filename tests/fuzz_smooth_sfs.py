"""The export stage of `smooth --index --sfs` (csrc/bam_smooth.hip: sm_sfs_flag_kernel, sm_sfs_scatter_kernel,
sm_sfs_nt6_kernel) in the rotation of tests/fuzz_gpu.py:

    python -m tests.fuzz_smooth_sfs --what smooth_sfs --minutes 2 --seed 1        (or any list of tests.fuzz_gpu's names)

A random BAM -- CIGARs with indels on both sides of the 20 bp threshold, clips, reads shorter than 100 bases, XF / HP tags
of every integer type already present, unmapped / secondary / low-MAPQ records -- goes through svdss_bam_smooth_run with
svdss_bam_smooth_set_search, batch by batch, and every batch is finished by svdss_bam_smooth_search.  The checker is a
host twin: it inflates the BGZF members the same runs produced (S), walks the rebuilt records as `search` would (flags,
l_seq >= 100, qname, HP, XF), unpacks their 4-bit bases to nt6 and searches them with the oracle.  Names, HP, which reads
are searched and every SFS must agree.  Then S itself is checked (check_smoothed_stream): the mirror of smoother.cpp applied to
the input's records must give the records of S -- so the 19 / 20 / 21 bp indels count for the smoothing, too."""
import ctypes as C
import struct
import zlib

import numpy as np

import svdss_amd
from svdss_amd import bamdev, bgzf, synth
from svdss_amd._lib import SVDSS_BAM_PUTATIVE, SVDSS_SFS_ASSEMBLE, SvdssError, lib
from tests import bam_writer, fuzz_gpu
from tests import oracle_lib as O
from tests.fuzz_gpu import Mismatch, _dump


class Smoothed(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_kept", C.c_int64), ("match_mismatch", C.POINTER(C.c_int64)), ("fits", C.POINTER(C.c_uint8)),
                ("out_bytes", C.c_int64), ("bgzf", C.POINTER(C.c_uint8)), ("bgzf_bytes", C.c_int64), ("n_xf", C.c_int64 * 4),
                ("inflate_kernel_ms", C.c_double), ("stage_ms", C.c_double * 8)]


def _check(rc, what):
    if rc:
        raise SvdssError(rc, what)


def smooth_and_search(index, contigs_ascii, data, min_mapq, acc, putative, assemble, batch_bytes):
    """(S = the BGZF members of the smoothed stream, [(name, hp, None | [(qs, len)])] of the reads `search` would deal)"""
    blocks = bgzf.bgzf_blocks(data)
    n_ref, skip = bamdev.bam_header(data, blocks)
    raw_head = b""
    for coff, clen, isize, _ in blocks:
        raw_head += zlib.decompress(bytes(data[coff:coff + clen]), -15)
        if len(raw_head) >= skip:
            break
    cat = np.frombuffer("".join(contigs_ascii).encode(), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs_ascii])]).astype(np.int64)
    ref, sm, stream, batch = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    tid_map = np.arange(n_ref, dtype=np.int32)
    comp = np.frombuffer(bytes(data), dtype=np.uint8)
    S, out = bytearray(), []
    flags = (SVDSS_SFS_ASSEMBLE if assemble else 0) | (SVDSS_BAM_PUTATIVE if putative else 0)
    try:
        _check(lib.svdss_ref_upload(cat.ctypes.data, off.ctypes.data, len(contigs_ascii), 0, C.byref(ref)), "svdss_ref_upload")
        _check(lib.svdss_bam_smooth_create(ref, tid_map.ctypes.data, n_ref, min_mapq, C.byref(sm)), "svdss_bam_smooth_create")
        _check(lib.svdss_bam_smooth_set_search(sm, flags, None), "svdss_bam_smooth_set_search")
        _check(lib.svdss_bam_stream_create(n_ref, C.byref(stream)), "svdss_bam_stream_create")
        head = np.frombuffer(raw_head[:skip], dtype=np.uint8)
        _check(lib.svdss_bam_stream_set_output_prefix(stream, head.ctypes.data, len(head)), "svdss_bam_stream_set_output_prefix")
        groups, cur, accb = [], [], 0
        for b in blocks:
            cur.append(b)
            accb += b[2]
            if accb >= batch_bytes:
                groups.append(cur)
                cur, accb = [], 0
        groups.append(cur)
        for seq, g in enumerate(groups):
            rec = np.zeros(max(1, len(g)), dtype=[("coff", "<i8"), ("clen", "<i4"), ("isize", "<i4"), ("uoff", "<i8")])
            crc = np.zeros(max(1, len(g)), dtype=np.uint32)
            for i, b in enumerate(g):
                rec[i] = (b[0], b[1], b[2], 0)
                crc[i] = b[3]
            rc = lib.svdss_bam_smooth_run(stream, seq, 1 if seq == len(groups) - 1 else 0, skip if seq == 0 else 0, sm, C.c_double(acc), None, 0, 1,
                                          (C.c_void_p * 1)(comp.ctypes.data), (C.c_int64 * 1)(len(comp)), (C.c_void_p * 1)(rec.ctypes.data),
                                          (C.c_void_p * 1)(crc.ctypes.data), (C.c_int64 * 1)(len(g)), C.byref(batch))
            if rc:
                raise SvdssError(rc, "svdss_bam_smooth_run: " + (lib.svdss_bam_batch_error(batch) or b"").decode())
            sr = Smoothed()
            _check(lib.svdss_bam_batch_smoothed(batch, C.byref(sr)), "svdss_bam_batch_smoothed")
            S += C.string_at(sr.bgzf, sr.bgzf_bytes) if sr.bgzf_bytes else b""
            grp = C.c_int64(0)
            _check(lib.svdss_bam_batch_parked(batch, C.byref(grp), None, None), "svdss_bam_batch_parked")
            if grp.value == -1:
                _check(lib.svdss_bam_smooth_search(batch, index._h), "svdss_bam_smooth_search")
            elif grp.value != -2:
                raise Mismatch(f"a batch without a park says group {grp.value}")
            r = bamdev.BamResult()
            _check(lib.svdss_bam_batch_result(batch, C.byref(r)), "svdss_bam_batch_result")
            n = r.n_slots
            name_off = np.ctypeslib.as_array(r.name_off, shape=(n + 1,)).copy() if n else np.zeros(1, np.int32)
            names = C.string_at(r.names, int(name_off[-1])) if n else b""
            counts = np.ctypeslib.as_array(r.counts, shape=(r.n_searched,)).copy() if r.n_searched else np.zeros(0, np.int64)
            first = np.concatenate([[0], np.cumsum(counts)])
            for i in range(n):
                k = int(r.sidx[i])
                sfs = None if k < 0 else [(int(r.qs[j]), int(r.len[j])) for j in range(int(first[k]), int(first[k + 1]))]
                out.append((names[name_off[i]:name_off[i + 1]].decode(), int(r.hp[i]), sfs))
    finally:
        if batch:
            lib.svdss_bam_batch_free(batch)
        if stream:
            lib.svdss_bam_stream_free(stream)
        if sm:
            lib.svdss_bam_smooth_free(sm)
        if ref:
            lib.svdss_ref_free(ref)
    return bytes(S), out


_INT = {"c": ("<b", 1), "C": ("<B", 1), "s": ("<h", 2), "S": ("<H", 2), "i": ("<i", 4), "I": ("<I", 4)}


def aux_int(aux, tag):
    """BamReader::aux_int: the first integer tag of that name; anything unexpected ends the walk with "absent"."""
    p = 0
    while p + 3 <= len(aux):
        t, ty = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if ty in "AcC":
            sz = 1
        elif ty in "sS":
            sz = 2
        elif ty in "iIf":
            sz = 4
        elif ty in "ZH":
            z = aux.find(b"\0", p)
            sz = (len(aux) if z < 0 else z) - p + 1
        elif ty == "B":
            if p + 5 > len(aux):
                return None
            sz = 5 + {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(aux[p]), 4) * struct.unpack_from("<I", aux, p + 1)[0]
        else:
            return None
        if sz > len(aux) - p:
            return None
        if t == tag:
            return struct.unpack_from(_INT[ty][0], aux, p)[0] if ty in _INT else None
        p += sz
    return None


NT6_OF_NIBBLE = np.array([5, 1, 2, 5, 3, 5, 5, 5, 4, 5, 5, 5, 5, 5, 5, 5], dtype=np.uint8)   # "=ACMGRSVTWYHKDBN" through seq_nt6_table


def host_twin(S, putative):
    """[(name, hp, None | nt6 bases)] of the reads `search` deals from S, in file order"""
    raw = b"".join(zlib.decompress(S[c:c + n], -15) for c, n, _, _ in bgzf.bgzf_blocks(S))
    l_text = struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, 8 + l_text)[0]
    p = 12 + l_text
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", raw, p)[0]
    out = []
    while p + 4 <= len(raw):
        bs = struct.unpack_from("<i", raw, p)[0]
        l_name, n_cig, flag, l_seq = raw[p + 12], *struct.unpack_from("<HHi", raw, p + 16)
        sq = p + 36 + l_name + 4 * n_cig
        ax = sq + (l_seq + 1) // 2 + l_seq
        if not flag & (4 | 256 | 2048) and l_seq >= 100:
            aux = raw[ax:p + 4 + bs]
            xf, hp = aux_int(aux, b"XF") or 0, aux_int(aux, b"HP") or 0
            bases = None
            if not (putative and xf != 0):
                pk = np.frombuffer(raw, dtype=np.uint8, count=(l_seq + 1) // 2, offset=sq)
                bases = NT6_OF_NIBBLE[np.stack([pk >> 4, pk & 15], axis=1).reshape(-1)[:l_seq]]
            out.append((raw[p + 36:p + 36 + l_name - 1].decode(), int(np.int32(hp)), bases))
        p += 4 + bs
    return out


def _random_bam(rng, contigs):
    recs = []
    for k in range(int(rng.integers(20, 400))):
        tid = int(rng.integers(0, len(contigs)))
        c = contigs[tid]
        want = int(rng.choice([int(rng.integers(2, 100)), int(rng.integers(100, 140)), int(rng.integers(140, 3000))], p=[0.15, 0.15, 0.7]))
        pos = int(rng.integers(0, max(1, len(c) - 1)))
        err = float(rng.choice([0.0, 0.003, 0.05]))
        cig, seq, rp = [], [], pos
        if rng.random() < 0.3:
            l = int(rng.integers(1, 200)); cig.append(("S", l)); seq.append(rng.integers(1, 5, size=l).astype(np.uint8))
        while sum(len(s) for s in seq) < want and rp < len(c) - 1:
            l = int(min(rng.integers(1, 500), len(c) - rp))
            m = c[rp:rp + l].copy()
            e = rng.random(l) < err
            m[e] = (m[e] % 4) + 1
            cig.append(("M", l)); seq.append(m); rp += l
            u = rng.random()
            if u < 0.25:
                l = int(rng.choice([1, 19, 20, 21, int(rng.integers(22, 300))])); cig.append(("I", l)); seq.append(rng.integers(1, 5, size=l).astype(np.uint8))
            elif u < 0.5 and rp + 400 < len(c):
                l = int(rng.choice([1, 19, 20, 21, int(rng.integers(22, 300))])); cig.append(("D", l)); rp += l
        if cig[-1][0] != "M":
            cig.pop() if cig[-1][0] == "D" else None
        if rng.random() < 0.3:
            l = int(rng.integers(1, 200)); cig.append(("S", l)); seq.append(rng.integers(1, 5, size=l).astype(np.uint8))
        if not seq or cig[-1][0] == "D":
            continue
        s = np.concatenate(seq)
        if len(s) < 2:
            continue
        tags = []
        u = rng.random()
        if u < 0.5:
            ty = str(rng.choice(list("cCsSiI")))
            tags.append(("HP", ty, int(rng.integers(-3, 4)) if ty in "csi" else int(rng.integers(0, 4))))
        if rng.random() < 0.3:
            tags.insert(int(rng.integers(0, len(tags) + 1)), ("XF", str(rng.choice(list("CsiI"))), int(rng.integers(0, 250))))
        if rng.random() < 0.2:
            tags.insert(int(rng.integers(0, len(tags) + 1)), ("ZZ", "Z", "text"))
        flag = int(rng.choice([0, 16, 4, 256, 2048, 1024], p=[0.5, 0.3, 0.05, 0.05, 0.05, 0.05]))
        name = f"r{k:04d}" if rng.random() < 0.9 or not recs else f"r{int(rng.integers(0, k)):04d}"
        qual = bytes(rng.integers(1, 60, size=len(s)).astype(np.uint8))
        recs.append((tid, pos, bam_writer.record(name, flag, tid, pos, int(rng.choice([0, 19, 20, 60])), cig, synth.to_ascii(s), tags, qual)))
    recs.sort(key=lambda r: (r[0], r[1]))
    return bam_writer.bam([(f"c{i}", len(c)) for i, c in enumerate(contigs)], [r[2] for r in recs])


def fuzz_smooth_sfs(rng, out_dir, it):
    contigs = [rng.integers(1, 5, size=int(rng.integers(3000, 60000))).astype(np.uint8) for _ in range(int(rng.integers(1, 4)))]
    data = _random_bam(rng, contigs)
    putative, assemble = bool(rng.random() < 0.6), bool(rng.random() < 0.5)
    acc = float(rng.choice([0.0, 0.001, 0.01, 1.0]))
    batch_bytes = int(rng.choice([1 << 12, 1 << 16, 1 << 28]))
    ix = svdss_amd.FMDIndex.build(contigs).to_device(0)
    try:
        S, got = smooth_and_search(ix, [synth.to_ascii(c) for c in contigs], data, 20, acc, putative, assemble, batch_bytes)
    finally:
        ix.close()
    want = host_twin(S, putative)
    where = lambda: _dump(out_dir, f"smooth_sfs_{it}", bam=np.frombuffer(data, np.uint8), contigs=contigs, acc=acc, putative=putative, batch=batch_bytes)   # noqa: E731
    if [(n, h, s is None) for n, h, s in got] != [(n, h, b is None) for n, h, b in want]:
        raise Mismatch("names / HP / searched flags of the exported reads differ from the smoothed records': " + where())
    reads = [b for _, _, b in want if b is not None]
    if reads:
        flat, offs = svdss_amd.pack_reads(reads)
        c, q, l, _ = O.OracleFMD.build(contigs).search_batch(flat, offs, assemble)
        first = np.concatenate([[0], np.cumsum(c)])
        k = 0
        for n, h, sfs in got:
            if sfs is None:
                continue
            if sfs != [(int(q[j]), int(l[j])) for j in range(int(first[k]), int(first[k + 1]))]:
                raise Mismatch(f"SFS of exported read {k} ({n}) differ from the oracle's on the smoothed record's bases: " + where())
            k += 1
    n_smoothed = check_smoothed_stream(S, data, contigs, 20, acc, where)
    return len(want), f"{len(want)} reads dealt, {len(reads)} searched, {len(S)} bytes of S, {n_smoothed} records as the mirror smooths them"


def check_smoothed_stream(S, data, contigs, min_mapq, acc, where):
    """Was S smoothed correctly?  The mirror of smoother.cpp (tests/mirror/smoother.py) applied to the input's records: the
    same records in the same order, XF, bases, qualities, CIGAR and aux block."""
    import gzip
    from tests.mirror import bamio, smoother
    names, _, alns = bamio.parse_bam(gzip.decompress(bytes(data)))
    _, _, got = bamio.parse_bam(b"".join(zlib.decompress(S[c:c + n], -15) for c, n, _, _ in bgzf.bgzf_blocks(S)))
    chrom = {n: synth.to_ascii(c) for n, c in zip(names, contigs)}
    kept = [a for a in alns if smoother.eligible(a, names, chrom, min_mapq)]
    if [g.qname for g in got] != [a.qname for a in kept]:
        raise Mismatch("the smoothed stream does not hold the records the filters keep, in their order: " + where())
    for g, a in zip(got, kept):
        xf, ns, nq, nc = smoother.smooth_read(a, a.qual, chrom[names[a.tid]], acc)
        if xf != 0:
            ns, nq, nc = a.seq, a.qual, a.cigar
        if (g.flag, g.tid, g.pos, g.mapq, g.seq, g.qual, g.cigar, g.aux) != (a.flag, a.tid, a.pos, a.mapq, ns, nq, list(nc), smoother.update_xf(a.aux, xf)):
            raise Mismatch(f"record {a.qname} (XF {xf} by the mirror) is not smoothed as the mirror smooths it: " + where())
    return len(got)


fuzz_gpu.FUZZERS["smooth_sfs"] = fuzz_smooth_sfs

if __name__ == "__main__":
    fuzz_gpu.main()
