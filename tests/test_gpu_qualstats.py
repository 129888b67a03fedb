"""GPU parity of BasePairQualStats (qualstats.hip, KBQ k_readpos_stats) with the tests' Python restatement of
alignments/BasePairQualityStatisticsCalculator.java (tests/qualstats_restatement.py): the whole report text must be
identical (integer counts: exact in any order)."""
import ctypes
import math
import os
import subprocess

import pytest

import pysynth
import qualstats_cases
import qualstats_restatement
import read_shapes
from ngsepcore_amd import BasePairQualityStatisticsCalculator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ngsepcore_amd", "lib", "ngsep-amd")


def _bam(sam):
    return pysynth.sam_to_bam(sam, sam[:-4] + ".bam")


def _calc(fa, min_mq=20):
    calc = BasePairQualityStatisticsCalculator()
    calc.setGenome(fa)
    calc.setMinMQ(min_mq)
    return calc


def path_b(fa, bams, out, min_mq=20):
    """run(): the C++ reader over the files, the report written by the library"""
    with _calc(fa, min_mq) as calc:
        calc.setInputFiles(bams)
        calc.setOutputFile(out)
        calc.run()
        txt = open(out).read()
        assert calc.printStatistics() == txt
        return txt


def path_a(fa, bam, batch_reads, min_mq=20):
    """the same records handed over as character batches of batch_reads alignments"""
    with _calc(fa, min_mq) as calc:
        calc.processFileBatches(bam, batch_reads)
        return calc.printStatistics()


def test_hand_made_case_path_b_path_a_cli(tmp_path):
    fa, sam = qualstats_cases.hand_case(tmp_path)
    bam = _bam(sam)
    want = qualstats_cases.HAND_REPORT
    assert qualstats_restatement.run([sam], fa).report() == want
    assert path_b(fa, [bam], os.path.join(str(tmp_path), "b.txt")) == want
    assert path_a(fa, bam, 1 << 20) == want
    assert path_a(fa, bam, 2) == want
    out = os.path.join(str(tmp_path), "cli.txt")
    subprocess.run([EXE, "BasePairQualStats", "-r", fa, "-o", out, bam], check=True, timeout=60)
    assert open(out).read() == want
    r = subprocess.run([EXE, "BasePairQualStats", "-r", fa, "-minMQ", "0", bam], check=True, timeout=60, capture_output=True, text=True)
    assert r.stdout == qualstats_restatement.run([sam], fa, min_mq=0).report()


def test_hand_made_case_as_a_host_built_batch():
    """Path A from a host with its own reader: the hand-made case's alignments as a character batch (lower-case
    characters among them, 0x1000 on the alignments its reader found multiple), no BAM and no C++ reader involved"""
    ops = "HDIMPNSX"                                           # NGSEP item codes, length * 8 + code
    recs = [(1, 0, [(8, "M")], "ACGTacga"),                    # r1
            (1, 0x1000, [(4, "M")], "NCGT"),                   # r3: MAPQ 5 < minMQ
            (3, 0x100 | 0x1000, [(4, "M")], "gtaa"),           # r4: secondary
            (5, 0x10, [(2, "S"), (4, "M"), (2, "I"), (2, "M")], "TTACGAGGAC"),   # r2
            (11, 0, [(3, "M"), (1, "D"), (3, "M")], "GTAGTc")]                   # r6: NH 1
    n = len(recs)
    cig = [l * 8 + ops.index(o) for _, _, c, _ in recs for l, o in c]
    bases = "".join(r[3] for r in recs).encode()
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    cig_n = [len(r[2]) for r in recs]
    seq_len = [len(r[3]) for r in recs]
    keep = dict(seq_id=(i32 * n)(*[0] * n), first=(i32 * n)(*[r[0] for r in recs]), flags=(i32 * n)(*[r[1] for r in recs]),
                read_group=(i32 * n)(*[-1] * n), cigar_off=(i64 * n)(*[sum(cig_n[:k]) for k in range(n)]),
                cigar_n=(i32 * n)(*cig_n), cigar=(i32 * len(cig))(*cig),
                seq_off=(i64 * n)(*[sum(seq_len[:k]) for k in range(n)]), seq_len=(i32 * n)(*seq_len))
    from ngsepcore_amd._lib import NgsepReadBatch
    batch = NgsepReadBatch(n_reads=n, bases=bases, quals=None, has_quals=None, **keep)
    # the same five alignments 210,000 times over in one batch: 1,050,000 records, more than one launch takes (2^20), so
    # the batch is cut in two; every record still points at the first copy's CIGAR items and characters
    import numpy as np
    reps = 210000
    big = {k: np.tile(np.ctypeslib.as_array(keep[k]), reps) for k in ("seq_id", "first", "flags", "read_group", "cigar_off",
                                                                      "cigar_n", "seq_off", "seq_len")}
    ptr = {k: v.ctypes.data_as(ctypes.POINTER(i64 if v.dtype == np.int64 else i32)) for k, v in big.items()}
    big_batch = NgsepReadBatch(n_reads=n * reps, bases=bases, quals=None, has_quals=None, cigar=keep["cigar"], **ptr)
    want = qualstats_restatement.QualStats()
    with BasePairQualityStatisticsCalculator() as calc:
        calc.contigs = [("c1", ("ACGT" * 10).encode())]
        calc.processBatches([batch])
        assert calc.printStatistics() == qualstats_cases.HAND_REPORT
        calc.processBatches([batch])                           # counts accumulate until cleared
        assert calc.getTotalBases() == 54 and calc.mismatches[7] == 2
        calc.init()
        calc.processBatches([big_batch])
        want.mismatches = [0, 0, 0, reps, reps, reps, 0, reps, 0, 0]
        want.mismatches_unique = [0, 0, 0, 0, reps, reps, 0, reps, 0, 0]
        want.alns_by_length = [0, 0, 0, 2 * reps, 0, reps, 0, reps, 0, reps]
        want.unique_by_length = [0, 0, 0, 0, 0, reps, 0, reps, 0, reps]
        want.total_alignments, want.reads_unique, want.total_bases, want.bases_unique = 5 * reps, 3 * reps, 27 * reps, 20 * reps
        assert calc.printStatistics() == want.report()


@pytest.fixture(scope="module")
def lanes(tmp_path_factory):
    d = tmp_path_factory.mktemp("lanes")
    fa, sam = qualstats_cases.lane_shapes(d)
    text = open(sam).read()
    for what in ("S", "H", "I", "D", "N", "=", "X", "P"):
        assert any(what in l.split("\t")[5] for l in text.splitlines() if not l.startswith("@")), what
    return fa, sam, _bam(sam)


@pytest.mark.parametrize("min_mq", [20, 30])
def test_lane_boundary_shapes(tmp_path, lanes, min_mq):
    fa, sam, bam = lanes
    st = qualstats_restatement.run([sam], fa, min_mq=min_mq)
    want = st.report()
    assert st.total_alignments > 200 and 0 < st.reads_unique < st.total_alignments and sum(st.mismatches) > 200
    assert len(st.mismatches) == 129
    assert path_b(fa, [bam], os.path.join(str(tmp_path), "b.txt"), min_mq) == want
    assert path_a(fa, bam, 1 << 20, min_mq) == want


def test_long_read_global_bins(tmp_path):
    """50,000 read positions: past any LDS-resident bins, and the result arrays grow"""
    fa, sam = qualstats_cases.long_read(tmp_path)
    bam = _bam(sam)
    st = qualstats_restatement.run([sam], fa)
    want = st.report()
    assert len(st.mismatches) == 50000
    # reverse strand: the mismatches at j = 49999, 49990 and 3, 0 are the report's positions 1, 10 and 49997, 50000
    for i in (0, 9, 49996, 49999):
        assert st.mismatches[i] >= 1, i
    assert path_b(fa, [bam], os.path.join(str(tmp_path), "b.txt")) == want
    # three alignments a batch: the long read arrives after 100-base reads were counted (the arrays grow with counts in them)
    assert path_a(fa, bam, 3) == want


def test_real_read_shapes(tmp_path):
    d = str(tmp_path)
    sam0, fa = os.path.join(d, "all.sam"), os.path.join(d, "s.fa")
    read_shapes.make_sam(sam0, fa, seed=11, depth=8, lengths=(40000, 25000))
    # SEQ '*' records stay out of the parity data (the reference fails on them) ...
    sam = os.path.join(d, "s.sam")
    n_star = 0
    with open(sam, "w") as f:
        for l in open(sam0):
            star = not l.startswith("@") and l.split("\t")[9] == "*" and not int(l.split("\t")[1]) & 4
            n_star += star
            if not star:
                f.write(l)
    assert n_star > 0
    st = qualstats_restatement.run([sam], fa, skip_seq_star=False)
    want = st.report()
    assert st.total_alignments > 2000 and len(st.mismatches) >= 5000
    assert path_b(fa, [_bam(sam)], os.path.join(d, "b.txt")) == want
    # ... and with them in the file the product skips them, as documented (a repeated record is a verbatim copy, so
    # dropping the '*' lines leaves every other record's isSameAlignment outcome as it was)
    assert path_b(fa, [_bam(sam0)], os.path.join(d, "b0.txt")) == want


def test_several_files_and_small_batches(tmp_path):
    d = str(tmp_path)
    fa, sam1 = qualstats_cases.long_read(tmp_path, seed=5, length=9000, long_len=3000)
    # a second file on the same genome: short reads only
    sam2 = os.path.join(d, "short.sam")
    with open(sam2, "w") as f:
        for l in open(sam1):
            if l.startswith("@") or l.split("\t")[0] != "long":
                f.write(l.replace("100M", "60M40S") if not l.startswith("@") else l)
    bam1, bam2 = _bam(sam1), _bam(sam2)
    both = qualstats_restatement.run([sam2, sam1], fa)
    one, two = qualstats_restatement.run([sam1], fa), qualstats_restatement.run([sam2], fa)
    assert path_b(fa, [bam2, bam1], os.path.join(d, "both.txt")) == both.report()
    # the sum of the two single-file runs: the short file first, so the longer reads come to arrays already in use
    with _calc(fa) as calc:
        calc.processFile(bam2)
        assert calc.printStatistics() == two.report()
        calc.processFile(bam1)
        assert calc.printStatistics() == both.report()
        n = len(both.mismatches)
        assert calc.mismatches == [a + b for a, b in zip(one.mismatches, two.mismatches + [0] * n)]
        assert calc.getTotalBases() == one.total_bases + two.total_bases
        calc.init()
        assert calc.printStatistics() == "\nAlignments\t0\t0\nBases\t0\t0\n"
    # one file in batches of two alignments: a longer read arrives in a later batch than a shorter one
    assert path_a(fa, bam1, 2) == one.report()


def test_python_class_percentages_and_clear(tmp_path, lanes):
    fa, sam, bam = lanes
    st = qualstats_restatement.run([sam], fa)
    with _calc(fa) as calc:
        calc.processFile(bam)
        assert (calc.getTotalAlignments(), calc.getReadsUniqueMapping(), calc.getTotalBases(), calc.getBasesUniqueMapping()) == \
               (st.total_alignments, st.reads_unique, st.total_bases, st.bases_unique)
        for unique in (False, True):
            got, want = calc.calculatePercentages(unique), st.percentages(unique)
            assert len(got) == len(want) == 129
            assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(got, want))
        s = calc._session()
        assert s._lib.ngsep_clear_qualstats(s._ctx) == 0
        n, tot = ctypes.c_int64(-1), (ctypes.c_int64 * 4)(1, 1, 1, 1)
        assert s._lib.ngsep_fetch_qualstats(s._ctx, None, None, None, None, 0, ctypes.byref(n), tot) == 0
        assert n.value == 0 and list(tot) == [0, 0, 0, 0]
        # and the counters count again from zero
        calc.processFile(bam)
        assert calc.printStatistics() == st.report()
