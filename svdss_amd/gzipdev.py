"""Plain single-stream gzip inflated on the GPU: Python binding of svdss_gzip_stream_* (csrc/gzip_stream.hip).  The host
side here does what the binary's source thread does (csrc/search_host.cpp): hand the file over window by window, take the
text of every run, and -- where the unit declines -- read on from the carried state with zlib (svdss_gzip_stream_host_tail:
csrc/gzip_stream.h's GzHostTail)."""
import ctypes as C

import numpy as np

from ._lib import SvdssError, lib

DECLINE_REASONS = {0: "", 1: "not a gzip header", 2: "no dynamic block start in the window", 3: "no whole block in the window",
                   4: "an invalid code", 5: "trailing bytes that are no gzip header"}


class GzipResult(C.Structure):
    _fields_ = [("text", C.POINTER(C.c_uint8)), ("d_text", C.c_void_p), ("text_bytes", C.c_int64),
                ("windows", C.c_int64), ("n_chunks", C.c_int64), ("chunks_on_chain", C.c_int64), ("chunks_merged", C.c_int64),
                ("false_starts", C.c_int64), ("members_finished", C.c_int64), ("device_bytes", C.c_int64),
                ("ended", C.c_int32), ("declined", C.c_int32),
                ("byte_pos", C.c_int64), ("bit", C.c_int32), ("in_member", C.c_int32), ("want_trailer", C.c_int32),
                ("crc", C.c_uint32), ("count", C.c_uint64), ("dict", C.POINTER(C.c_uint8)), ("dict_len", C.c_int32),
                ("find_ms", C.c_double), ("measure_ms", C.c_double), ("decode_ms", C.c_double), ("resolve_ms", C.c_double)]


class GzipError(SvdssError):
    """A damaged stream: .detail says what is wrong with it."""
    detail = ""


def _fail(stream, rc, where):
    e = GzipError(rc, where)
    e.detail = (lib.svdss_gzip_stream_error(stream) or b"").decode()
    e.args = (f"{e.args[0]}: {e.detail}",)
    return e


def inflate(data, chunk_bytes=256 << 10, window_bytes=64 << 20, device=0):
    """`data`: the bytes of a gzip file.  (its text, counters): the counters of svdss_gzip_result_t, the window count,
    `declined` (0 or the reason) with `declined_at` (the byte of the file where the host took over) and `host_bytes`."""
    data = bytes(data)
    comp = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    stream = C.c_void_p()
    rc = lib.svdss_gzip_stream_create(device, chunk_bytes, C.byref(stream))
    if rc:
        raise SvdssError(rc, "svdss_gzip_stream_create")
    out = []
    r = GzipResult()
    host_bytes = 0
    try:
        pos, win = 0, window_bytes
        while True:
            n = min(win, len(data) - pos)
            is_last = 1 if pos + n >= len(data) else 0
            used = C.c_int64(0)
            rc = lib.svdss_gzip_stream_run(stream, comp.ctypes.data + pos, n, is_last, C.byref(used))
            if rc:
                raise _fail(stream, rc, "svdss_gzip_stream_run")
            lib.svdss_gzip_stream_result(stream, C.byref(r))
            if r.text_bytes:
                out.append(C.string_at(r.text, r.text_bytes))
            pos += used.value
            assert r.byte_pos == pos
            if r.declined:
                rc = lib.svdss_gzip_stream_host_tail(stream, comp.ctypes.data + pos, len(data) - pos)
                if rc:
                    raise _fail(stream, rc, "svdss_gzip_stream_host_tail")
                t = GzipResult()
                lib.svdss_gzip_stream_result(stream, C.byref(t))
                if t.text_bytes:
                    out.append(C.string_at(t.text, t.text_bytes))
                host_bytes = t.text_bytes
                break
            if r.ended:
                break
            if used.value == 0 and not r.text_bytes:
                if is_last:
                    raise _fail(stream, 3, "svdss_gzip_stream_run: truncated stream")
                win *= 2          # (a header longer than the window)
            else:
                win = window_bytes
        stats = {k: getattr(r, k) for k in ("windows", "n_chunks", "chunks_on_chain", "chunks_merged", "false_starts",
                                              "members_finished", "device_bytes", "declined", "find_ms", "measure_ms",
                                              "decode_ms", "resolve_ms")}
        stats["declined_at"] = pos if r.declined else None
        stats["declined_bit"] = r.bit if r.declined else None
        stats["host_bytes"] = host_bytes
    finally:
        lib.svdss_gzip_stream_free(stream)
    return b"".join(out), stats
