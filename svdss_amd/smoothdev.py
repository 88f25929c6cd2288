"""svdss_smooth_batch (csrc/place.hip, smooth_kernel: one wavefront per record) from Python, for the tests that compare the
kernel with the mirror (tests/test_smooth_edges_gpu.py): the CIGAR walk of the host pipeline of `SVDSS smooth`, on records
given as lists.  A test helper, not a fast path: the chromosomes go up and are freed again in every call.  The kernel has
no bounds of its own -- smooth_host.cpp hands it only records that fit (cigar_fits) and sizes every record's output by its
CIGAR -- so this wrapper refuses what does not fit and sizes the output the same way."""
import ctypes as C

import numpy as np

from ._lib import SvdssError, lib


def cigar_spans(cigar):
    """(reference bases, read bases) the CIGAR words cover up to the first operation that is not M = X I D S"""
    rl = ql = 0
    for w in cigar:
        l, op = int(w) >> 4, int(w) & 0xf
        if op in (0, 7, 8):
            rl += l
            ql += l
        elif op in (1, 4):
            ql += l
        elif op == 2:
            rl += l
        else:
            break
    return rl, ql


def smooth_batch(contigs_ascii, tid, pos, cigars, seq4, quals, device=0):
    """contigs_ascii: the chromosomes (str, upper case); per record: its chromosome, its position, its CIGAR (uint32 words),
    its packed bases (bytes, two per byte) and its qualities (bytes, one per base).  Returns one dict per record: length,
    cigar (uint32 words), seq4 (packed bases), qual, matches, mismatches, ignore ("nothing interesting")."""
    n = len(tid)
    if not (len(pos) == len(cigars) == len(seq4) == len(quals) == n):
        raise ValueError("one entry per record in every list")
    if n == 0:
        return []
    cig_off, s4_off, q_off, cap_off = [0], [], [], [0]
    s4_bytes = q_bytes = 0
    for k in range(n):
        rl, ql = cigar_spans(cigars[k])
        l_seq = len(quals[k])
        if not 0 <= tid[k] < len(contigs_ascii) or pos[k] < 0 or pos[k] + rl > len(contigs_ascii[tid[k]]) or ql != l_seq or len(seq4[k]) != (l_seq + 1) // 2:
            raise ValueError(f"record {k} does not fit its chromosome or its CIGAR does not add up to the read")
        cig_off.append(cig_off[-1] + len(cigars[k]))
        s4_off.append(s4_bytes)
        s4_bytes += len(seq4[k])
        q_off.append(q_bytes)
        q_bytes += l_seq
        cap_off.append(cap_off[-1] + ((ql + rl + 1) & ~1))
    n_cig, cap = cig_off[-1], cap_off[-1]

    def arr(values, dtype, pad=0):
        a = np.zeros(len(values) + pad, dtype=dtype)
        a[:len(values)] = values
        return a

    a_tid, a_pos = arr(tid, np.int32), arr(pos, np.int32)
    a_lq = arr([len(q) for q in quals], np.int32)
    a_cig = arr([int(w) for c in cigars for w in c], np.uint32, pad=4)
    a_s4 = np.frombuffer(b"".join(bytes(s) for s in seq4) + bytes(16), dtype=np.uint8)
    a_q = np.frombuffer(b"".join(bytes(q) for q in quals) + bytes(16), dtype=np.uint8)
    a_cig_off, a_s4_off, a_q_off, a_cap_off = (arr(v, np.int64) for v in (cig_off, s4_off, q_off, cap_off))
    o4, oq = np.zeros(cap // 2 + 8, np.uint8), np.zeros(cap + 8, np.uint8)
    ocig = np.zeros(n_cig + 1 + 4, np.uint32)
    oncig, olen, onm, oign = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(2 * n, np.int64), np.zeros(n, np.uint8)
    cat = np.frombuffer("".join(contigs_ascii).encode(), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs_ascii])]).astype(np.int64)
    ref = C.c_void_p()
    rc = lib.svdss_ref_upload(cat.ctypes.data, off.ctypes.data, len(contigs_ascii), device, C.byref(ref))
    if rc:
        raise SvdssError(rc, "svdss_ref_upload")
    try:
        rc = lib.svdss_smooth_batch(ref, a_tid.ctypes.data, a_pos.ctypes.data, a_cig.ctypes.data, a_cig_off.ctypes.data, a_s4.ctypes.data,
                                    a_s4_off.ctypes.data, a_q.ctypes.data, a_q_off.ctypes.data, a_lq.ctypes.data, a_cap_off.ctypes.data, n,
                                    o4.ctypes.data, oq.ctypes.data, ocig.ctypes.data, oncig.ctypes.data, olen.ctypes.data, onm.ctypes.data,
                                    oign.ctypes.data)
        if rc:
            raise SvdssError(rc, "svdss_smooth_batch")
    finally:
        lib.svdss_ref_free(ref)
    out = []
    for k in range(n):
        ln, nc, c0 = int(olen[k]), int(oncig[k]), cap_off[k]
        out.append({"length": ln, "cigar": ocig[cig_off[k]:cig_off[k] + nc].copy(), "seq4": o4[c0 // 2:c0 // 2 + (ln + 1) // 2].tobytes(),
                    "qual": oq[c0:c0 + ln].tobytes(), "matches": int(onm[2 * k]), "mismatches": int(onm[2 * k + 1]), "ignore": bool(oign[k])})
    return out
