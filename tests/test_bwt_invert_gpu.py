"""svdss_bwt_strings on device 0 (csrc/bwt_invert.hip: rank blocks made from the BWT bytes on the GPU, then the marked LF
walks, a walker per lane, as a plain grid and with lane refill) against the host route, byte for byte: the collections and strides of
tests/bwt_invert_cases.py, both BWT forms, guard bytes around the output -- and one collection large enough for several
wavefronts to take walkers again and again, with refill and as a plain grid."""
import numpy as np
import pytest

import svdss_amd
from svdss_amd import synth
from tests import bwt_invert_cases as K
from tests.test_bwt_invert import EINVAL, EIO, ERANGE, flipped_bwt

pytestmark = pytest.mark.gpu
NAMES = sorted(K.collections())


@pytest.mark.parametrize("refill", ["0", "1"])
@pytest.mark.parametrize("name", NAMES)
def test_device_walk_equals_host_walk_at_every_stride(name, refill, monkeypatch):
    monkeypatch.setenv("SVDSS_INVERT_REFILL", refill)      # the plain grid (default) and the resident wavefronts
    for form, (bwt, _) in (("rope", K.rope_bwt(name)), ("own", K.own_bwt(name))):
        rc, want, m = K.raw_strings(bwt, -1, 64)
        assert rc == 0
        if form == "rope":
            assert want == [bytes(s) for s in K.collections()[name]]
        for k, stride in enumerate(K.STRIDES):
            rc, got, m_dev = K.raw_strings(bwt, 0, stride, shift=k % 4)
            assert rc == 0 and m_dev == m, (form, stride, rc)
            assert got == want, (form, stride)
    assert svdss_amd.bwt_strings_last()["route"] == "device"


def test_many_wavefronts_refill(monkeypatch):
    """400,000 rows: at stride 16 some 25,000 walkers for the resident wavefronts to take in turn; at the default stride four
    hundred; both equal to the host walk, with refill and as a plain grid"""
    ref = synth.make_reference([150000, 49000, 997], seed=91, repeat_frac=0.2, n_runs=(300,))
    ix = svdss_amd.FMDIndex.build(ref)
    bwt = ix.bwt()
    ix.close()
    assert len(bwt) == 2 * (150000 + 49000 + 997 + 3)
    rc, want, m = K.raw_strings(bwt, -1, 0)
    assert rc == 0 and m == 6 and sorted(want) == sorted([bytes(c) for c in ref] + [bytes(synth.revcomp(c)) for c in ref])
    for refill in ("1", "0"):
        monkeypatch.setenv("SVDSS_INVERT_REFILL", refill)
        for stride in (0, 16):
            rc, got, _ = K.raw_strings(bwt, 0, stride, shift=1)
            assert rc == 0 and got == want, (refill, stride)
            last = svdss_amd.bwt_strings_last()
            assert last["route"] == "device" and last["stride"] == (stride or 1024)
            print(f"refill={refill} stride={last['stride']} walkers={last['walkers']} blocks {last['blocks_ms']:.3f} ms, "
                  f"pass 1 {last['pass1_ms']:.3f} ms, pass 2 {last['pass2_ms']:.3f} ms")


def test_refusals_on_the_device(monkeypatch):
    for stride in (1, 7, 1 << 20):
        rc, got, _ = K.raw_strings(flipped_bwt(), 0, stride)
        assert rc == EIO and got is None
    bwt, strings = K.rope_bwt("one_record")
    six = bwt.copy()
    six[len(six) // 2] = 6
    assert K.raw_strings(six, 0, 0)[0] == EINVAL
    monkeypatch.setenv("SVDSS_INVERT_MAX_STEPS", "5")
    rc, got, m = K.raw_strings(bwt, 0, 1 << 20)
    assert rc == ERANGE and got is None and m == 1
    got = svdss_amd.bwt_strings(bwt, device=0, stride=1 << 20)          # the wrapper's caller gets them all the same
    assert [bytes(g) for g in got] == [bytes(s) for s in strings]
