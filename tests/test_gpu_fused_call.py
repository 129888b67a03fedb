"""KGP (kernels.hip k_gather_call): the survivors' gather and genotyping in one kernel, on hand-written piles.

Every case is a contig of a few thousand bases, all-reference but for its planted sites, so the queue KL hands
to the kernel is known exactly: K sites, each with a chosen column.  The GPU's VCF must equal the oracle's byte
for byte, and a session with prune_candidates=1 (KL -> KGP) must return exactly the records of one with
prune_candidates=0 (KQ -> KG k_gather_cols -> KP k_posterior, the unfused kernels of the same library).
The unmarked test runs the oracle alone and checks that the fixtures are what the GPU cases assume."""
import os
import random

import pytest

from helpers import gpu_params, gpu_vcf_bam, oracle_vcf
import pysynth
from ngsepcore_amd import GpuPileupSession

READ_LEN = 100
COL_CAP = 128          # entries of a site's LDS column: kKgpColCap (ngsepcore_amd/csrc/kernels.hip)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}
THIRD = {"A": "G", "C": "T", "G": "A", "T": "C"}


def _reference(length, seed=5):
    rnd = random.Random(seed)
    return "".join(rnd.choice("ACGT") for _ in range(length))


def pile(ref, positions, depth, base=None, qual=None, reverse=None):
    """depth reads of READ_LEN bases that all cover the 1-based positions (their starts spread over every start
    that does).  base(i, k, r) is read i's base at the k-th position (reference base r; default: the other
    allele in every second read, so a heterozygous site), qual(i, k) its quality character (default Q40),
    reverse(i) its strand (default: alternating in pairs, so both alleles come on both strands)."""
    lo = max(1, max(positions) - READ_LEN + 1)
    hi = min(min(positions), len(ref) - READ_LEN + 1)
    assert lo <= hi
    reads = []
    for i in range(depth):
        start = lo + i % (hi - lo + 1)
        seq = list(ref[start - 1:start - 1 + READ_LEN])
        q = ["I"] * READ_LEN
        for k, p in enumerate(positions):
            r = ref[p - 1]
            seq[p - start] = base(i, k, r) if base else (OTHER[r] if (i + k) % 2 == 0 else r)
            if qual:
                q[p - start] = qual(i, k)
        rev = reverse(i) if reverse else (i // 2) % 2 == 1
        reads.append((start, 16 if rev else 0, "".join(seq), "".join(q)))
    return reads


def write_case(tmpdir, length, piles):
    ref = _reference(length)
    fa = os.path.join(str(tmpdir), "c.fa")
    with open(fa, "w") as f:
        f.write(">ctg\n")
        for i in range(0, length, 60):
            f.write(ref[i:i + 60] + "\n")
    reads = sorted((r for p in piles for r in pile(ref, **p)), key=lambda r: r[0])
    sam = os.path.join(str(tmpdir), "c.sam")
    with open(sam, "w") as f:
        f.write(f"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:ctg\tLN:{length}\n")
        for n, (start, flag, seq, q) in enumerate(reads):
            f.write(f"r{n}\t{flag}\tctg\t{start}\t60\t{READ_LEN}M\t*\t0\t0\t{seq}\t{q}\n")
    return fa, sam


def _sites(k):
    return [dict(positions=[300 + 250 * i], depth=20) for i in range(k)]


def _low_quality_base(i, k, r):
    return "N" if i % 8 == 7 else (OTHER[r] if i % 2 == 0 else r)


# name -> (contig length, piles, options, {planted position: its DP})
CASES = {}
for _k in (0, 1, 2, 3, 4, 5, 9):        # an empty queue, a wave with 1-3 live sites, whole waves, a partial last wave
    CASES[f"sites{_k}"] = (3000, _sites(_k), {}, {300 + 250 * i: 20 for i in range(_k)})
for _d in (1, 2, 63, 64, 65, COL_CAP - 1, COL_CAP, COL_CAP + 1, 300):   # chunk edge, LDS column edge, deep
    # (one call of each allele is called hom-ref and reported nowhere: the two shallowest columns are all-alternative)
    CASES[f"depth{_d}"] = (3000, [dict(positions=[1500], depth=_d, base=(lambda i, k, r: OTHER[r]) if _d <= 2 else None)],
                           {}, {1500: _d})
CASES["lds_and_fallback"] = (3000, [dict(positions=[700], depth=20), dict(positions=[1100], depth=200)], {},
                             {700: 20, 1100: 200})                     # two sites of one wave, one on each path
CASES["position_edges"] = (3000, [dict(positions=[20], depth=20), dict(positions=[255, 256, 257], depth=20),
                                  dict(positions=[2980], depth=20)], {},
                           {20: 20, 255: 20, 256: 20, 257: 20, 2980: 20})   # a 256-position block's edge; both contig ends
CASES["triallelic"] = (3000, [dict(positions=[1500], depth=40,
                                   base=lambda i, k, r: OTHER[r] if i % 2 == 0 else THIRD[r])], {}, {1500: 40})
CASES["low_quality"] = (3000, [dict(positions=[1500], depth=40, base=_low_quality_base,
                                    qual=lambda i, k: "#" if i % 8 in (2, 3) else "I")], {}, {1500: 40})
CASES["strand"] = (3000, [dict(positions=[1500], depth=40, reverse=lambda i: i % 2 == 0)], {"calc_strand_bias": 1},
                   {1500: 40})                                         # every alternative call on the negative strand
CASES["quality_cap"] = (3000, [dict(positions=[1500], depth=40)], {"max_base_qs": 10}, {1500: 40})
CASES["ploidy1"] = (3000, [dict(positions=[700], depth=20, base=lambda i, k, r: OTHER[r]),
                           dict(positions=[1500], depth=20)], {"ploidy": 1}, {700: 20, 1500: 20})

# every read is admitted whatever its start, and a call of any quality is reported (depth 1 and 2 give low ones)
COMMON = {"max_alns_per_start": 0, "min_quality": 0}


def _vcf_sites(path):
    out = {}
    for l in open(path):
        if not l.startswith("#"):
            f = l.rstrip("\n").split("\t")
            out[int(f[1])] = (f[4], int(f[9].split(":")[f[8].split(":").index("DP")]))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixtures_are_the_planted_sites(tmp_path, name):
    """The oracle alone: each SAM yields exactly its planted sites, at the intended depth."""
    length, piles, opts, planted = CASES[name]
    fa, sam = write_case(tmp_path, length, piles)
    o, _, _ = oracle_vcf(tmp_path, fa, sam, **COMMON, **opts)
    got = _vcf_sites(o)
    assert {p: dp for p, (_, dp) in got.items()} == planted
    if name == "triallelic":
        assert "," in got[1500][0]                     # two alternative alleles


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_call(tmp_path, name):
    length, piles, opts, planted = CASES[name]
    opts = dict(COMMON, **opts)
    fa, sam = write_case(tmp_path, length, piles)
    bam = pysynth.sam_to_bam(sam, os.path.join(str(tmp_path), "c.bam"))
    o, _, _ = oracle_vcf(tmp_path, fa, sam, **opts)
    g, _ = gpu_vcf_bam(tmp_path, fa, bam, **opts)
    assert open(g, "rb").read() == open(o, "rb").read()
    res = []
    for prune in (1, 0):
        with GpuPileupSession(gpu_params(prune_candidates=prune, **opts)) as s:
            s.load_fasta(fa)
            s.processFileBatches(bam)
            res.append([(x.sequence, x.pos, x.gq, x.qual, tuple(x.counts), tuple(x.logc)) for x in s.getCalledVariants()])
    assert res[0] == res[1]
    assert [x[1] for x in res[0]] == sorted(planted)
