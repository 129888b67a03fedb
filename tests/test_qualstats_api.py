"""BasePairQualStats without a GPU: the tests' Python restatement of the command on the hand-made case, the new C entry
points and their argument checks (include/ngsep_gpu.h "BasePairQualityStatisticsCalculator")."""
import ctypes
import os

import pytest

import qualstats_cases
import qualstats_restatement
from ngsepcore_amd import _lib

NEW_SYMBOLS = ("ngsep_qualstats_bams", "ngsep_qualstats_alignments", "ngsep_fetch_qualstats", "ngsep_write_qualstats",
               "ngsep_clear_qualstats")


def test_restatement_on_the_hand_made_case(tmp_path):
    fa, sam = qualstats_cases.hand_case(tmp_path)
    st = qualstats_restatement.run([sam], fa)
    assert st.report() == qualstats_cases.HAND_REPORT
    assert (st.total_alignments, st.reads_unique, st.total_bases, st.bases_unique) == (5, 3, 27, 20)
    assert st.percentages(False)[3] == 100.0 / 5 and st.percentages(True)[3] == 0.0
    # at -minMQ 0 the MAPQ 5 record is unique too (isMultiple :289); the secondary one never is
    st0 = qualstats_restatement.run([sam], fa, min_mq=0)
    assert st0.report().endswith("\nAlignments\t5\t4\nBases\t27\t23\n")


def test_restatement_seq_star_is_the_reference_failure(tmp_path):
    """SEQ '*': the reference dies on read.length() (:191); the restatement raises unless told to skip, as the product does"""
    fa, sam = qualstats_cases.hand_case(tmp_path)
    with open(sam, "a") as f:
        f.write("\t".join(["star", "0", "c1", "20", "60", "8M", "*", "0", "0", "*", "*"]) + "\n")
    with pytest.raises(TypeError):
        qualstats_restatement.run([sam], fa, skip_seq_star=False)
    assert qualstats_restatement.run([sam], fa).report() == qualstats_cases.HAND_REPORT


def test_symbols_load():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    import ngsepcore_amd
    calc = ngsepcore_amd.BasePairQualityStatisticsCalculator()
    assert calc.getMinMQ() == 20
    for m in ("setInputFiles", "setOutputFile", "setGenome", "setMinMQ", "getTotalAlignments", "getTotalBases",
              "getReadsUniqueMapping", "getBasesUniqueMapping", "calculatePercentages", "run", "processFile"):
        assert callable(getattr(calc, m)), m


def _open():
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.ngsep_open(0, None, ctypes.byref(ctx)) == _lib.NGSEP_OK
    return lib, ctx


def test_no_reference_is_invalid(tmp_path):
    lib, ctx = _open()
    paths = (ctypes.c_char_p * 1)(os.path.join(str(tmp_path), "x.bam").encode())
    assert lib.ngsep_qualstats_bams(ctx, paths, 1, None) == _lib.NGSEP_E_INVALID
    assert b"reference genome is a required parameter" in lib.ngsep_last_error(ctx)
    batch = _lib.NgsepReadBatch()
    assert lib.ngsep_qualstats_alignments(ctx, ctypes.byref(batch)) == _lib.NGSEP_E_INVALID
    assert lib.ngsep_qualstats_bams(ctx, paths, 0, None) == _lib.NGSEP_E_INVALID
    lib.ngsep_close(ctx)


def test_empty_counts_fetch_write_clear(tmp_path):
    """Before any run: no rows, zero totals, the report's two total lines; no device is needed for that"""
    lib, ctx = _open()
    n, tot = ctypes.c_int64(-1), (ctypes.c_int64 * 4)(9, 9, 9, 9)
    assert lib.ngsep_fetch_qualstats(ctx, None, None, None, None, 0, ctypes.byref(n), tot) == _lib.NGSEP_OK
    assert n.value == 0 and list(tot) == [0, 0, 0, 0]
    out = os.path.join(str(tmp_path), "empty.txt")
    assert lib.ngsep_write_qualstats(ctx, out.encode()) == _lib.NGSEP_OK
    assert open(out).read() == "\nAlignments\t0\t0\nBases\t0\t0\n"
    assert lib.ngsep_clear_qualstats(ctx) == _lib.NGSEP_OK
    assert lib.ngsep_write_qualstats(ctx, os.path.join(str(tmp_path), "no", "dir.txt").encode()) == _lib.NGSEP_E_IO
    lib.ngsep_close(ctx)


@pytest.mark.skipif(_lib.load().ngsep_device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_device_fails_loudly(tmp_path):
    """With a reference and no MI355X a run is refused: there is no CPU fallback"""
    import pysynth
    from ngsepcore_amd import BasePairQualityStatisticsCalculator, NgsepError
    fa, sam = qualstats_cases.hand_case(tmp_path)
    bam = pysynth.sam_to_bam(sam, os.path.join(str(tmp_path), "hand.bam"))
    with BasePairQualityStatisticsCalculator() as calc:
        calc.setGenome(fa)
        calc.setInputFiles([bam])
        with pytest.raises(NgsepError) as e:
            calc.run()
        assert e.value.code == _lib.NGSEP_E_DEVICE
    lib, ctx = _open()
    assert lib.ngsep_set_reference(ctx, b"c1", b"ACGT" * 10, 40) == _lib.NGSEP_OK
    batch = _lib.NgsepReadBatch()
    assert lib.ngsep_qualstats_alignments(ctx, ctypes.byref(batch)) == _lib.NGSEP_E_DEVICE
    lib.ngsep_close(ctx)
