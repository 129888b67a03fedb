"""MultisampleVariantsDetector on populations of more than 255 samples: KPM's threads take the sample columns in
blocks of 256 (kernels.hip k_posterior_wide), the first stage's masks are ceil(S / 32) words, the host's stream keys
are 32-bit past 511 samples.  Bar, as tests/test_gpu_multisample.py: the population VCF text identical to the CPU
restatement's (oracle/ngsep_oracle.c ngo_run_mvd).

Every data set and its oracle VCF is made once per session and shared by the run paths of its case."""
import os
import subprocess
import sys

import pytest

from helpers import diff_vcf
import ngsep_oracle
import pool_data
import pysynth
from test_gpu_multisample import gpu_mvd, n_records, oracle_mvd, population

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (Synth arguments, records the oracle writes)
SNV_CASES = {
    # the no-sample column is the only column of the second block of 256
    256: (dict(custom_len=2000, seed=61, n_samples=256, depth=4, snv_rate=1e-2, quality_model=2), 9),
    # one real sample in the second block
    257: (dict(custom_len=2000, seed=62, n_samples=257, depth=4, snv_rate=1e-2, quality_model=2), 16),
    # 16-bit stream keys would wrap (512 * 128 == 65536); masks of 16 words; 5 records with more than 64 carriers
    512: (dict(custom_len=2000, seed=63, n_samples=512, depth=4, snv_rate=1e-2, quality_model=2), 17),
    # four sample blocks; S1000..S1023 sort between S100 and S101 (read-group index != sample index)
    1024: (dict(custom_len=3000, seed=52, n_samples=1024, depth=4, snv_rate=1e-2, quality_model=2), 27),
}
INDEL_CASE = (dict(custom_len=4000, seed=64, n_samples=300, depth=6, snv_rate=5e-3, indel_rate=2e-3), 27)

_cache = {}


def _dir(tmp_path_factory, key):
    return tmp_path_factory.mktemp(f"wide_{key}")


def _synth_case(tmp_path_factory, key, kw):
    if key not in _cache:
        d = _dir(tmp_path_factory, key)
        syn, fa, sam, rgs = population(d, genome=pysynth.CUSTOM, **kw)
        _cache[key] = (syn, fa, sam, rgs, oracle_mvd(d, fa, sam), d)
    return _cache[key]


def _check(o, g, want):
    d = diff_vcf(o, g)
    assert not d, "\n".join(d[:20])
    assert n_records(g) * 2 >= want


@pytest.mark.parametrize("one_stage", [False, True])
@pytest.mark.parametrize("staged", [False, True, "pipelined"])
@pytest.mark.parametrize("n", sorted(SNV_CASES))
def test_wide_population_snv(tmp_path, tmp_path_factory, monkeypatch, n, staged, one_stage):
    kw, want = SNV_CASES[n]
    syn, fa, sam, rgs, o, _ = _synth_case(tmp_path_factory, n, kw)
    if one_stage:
        monkeypatch.setenv("NGSEP_KPM_ONE_STAGE", "1")
    g, st = gpu_mvd(tmp_path, syn, rgs, staged=staged)
    _check(o, g, want)


def test_wide_population_one_bam_1024_read_groups(tmp_path, tmp_path_factory):
    """One file with 1,024 read groups: the header path of ngsep_call_population_bams without 1,024 descriptors."""
    from ngsepcore_amd import MultisampleVariantsDetector
    kw, want = SNV_CASES[1024]
    syn, fa, sam, rgs, o, _ = _synth_case(tmp_path_factory, 1024, kw)
    bam = pysynth.sam_to_bam(sam, os.path.join(str(tmp_path), "all.bam"))
    d = MultisampleVariantsDetector()
    d.setGenome(fa)
    d.setOutFilename(os.path.join(str(tmp_path), "gpu_b.vcf"))
    d.run([bam])
    _check(o, d.outFilename, want)


def _indel_case(tmp_path_factory):
    kw, want = INDEL_CASE
    syn, fa, sam, rgs, o, d = _synth_case(tmp_path_factory, "indel300", kw)
    if "indel300_bams" not in _cache:
        _cache["indel300_bams"] = syn.write_sample_bams(os.path.join(str(d), "pop"))
    return syn, fa, sam, rgs, o, _cache["indel300_bams"], want


def test_wide_population_indels_path_a(tmp_path, tmp_path_factory):
    """300 samples with indels: KPM's site-major pile of the realigner regions (mode 0) and the host region path"""
    syn, fa, sam, rgs, o, _, want = _indel_case(tmp_path_factory)
    g, st = gpu_mvd(tmp_path, syn, rgs, staged=False)
    _check(o, g, want)
    indels = [l for l in open(o) if not l.startswith("#") and len(l.split("\t")[3]) != len(l.split("\t")[4].split(",")[0])]
    assert len(indels) >= 3


@pytest.mark.parametrize("stream", [False, True])
def test_wide_population_indels_path_b(tmp_path, tmp_path_factory, monkeypatch, stream):
    """... through MultisampleVariantsDetector.run on 300 sample BAMs, the whole-file merge and the streaming merge"""
    from ngsepcore_amd import MultisampleVariantsDetector
    syn, fa, sam, rgs, o, bams, want = _indel_case(tmp_path_factory)
    assert len(bams) == 300
    if stream:
        monkeypatch.setenv("NGSEP_POP_STREAM", "1")
    d = MultisampleVariantsDetector()
    d.setGenome(fa)
    d.setOutFilename(os.path.join(str(tmp_path), "gpu_b.vcf"))
    d.run(bams)
    _check(o, d.outFilename, want)


def test_wide_population_indels_cli(tmp_path, tmp_path_factory):
    syn, fa, sam, rgs, o, bams, want = _indel_case(tmp_path_factory)
    cli = os.path.join(ROOT, "ngsepcore_amd", "lib", "ngsep-amd")
    out = os.path.join(str(tmp_path), "cli.vcf")
    subprocess.run([cli, "MultisampleVariantsDetector", "-r", fa, "-o", out] + bams, check=True)
    _check(o, out, want)


_FD_CHILD = r"""
import os, resource, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
from ngsepcore_amd import MultisampleVariantsDetector, NgsepError, _lib
fa, out, bams = sys.argv[2], sys.argv[3], sys.argv[4:]
d = MultisampleVariantsDetector()
d.setGenome(fa)
d.setOutFilename(out)
soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
resource.setrlimit(resource.RLIMIT_NOFILE, (64, hard))
try:
    d.run(bams)
except NgsepError as e:
    print("CODE", e.code, "IO" if e.code == _lib.NGSEP_E_IO else "OTHER")
    print("MSG", e)
    sys.exit(0)
print("NOERROR")
"""


def test_wide_population_too_many_open_files(tmp_path, tmp_path_factory):
    """300 sample files against a descriptor limit of 64: NGSEP_E_IO with the system's message and a file name, no
    VCF left (a host I/O error; in a fresh child process, whose limit it is)."""
    syn, fa, sam, rgs, o, bams, want = _indel_case(tmp_path_factory)
    out = os.path.join(str(tmp_path), "never.vcf")
    script = os.path.join(str(tmp_path), "child.py")
    with open(script, "w") as f:
        f.write(_FD_CHILD)
    r = subprocess.run([sys.executable, script, ROOT, fa, out] + bams, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "CODE" in r.stdout and " IO" in r.stdout, r.stdout + r.stderr
    msg = [l for l in r.stdout.splitlines() if l.startswith("MSG")][0]
    assert os.strerror(24) in msg                       # EMFILE: "Too many open files"
    assert ".bam" in msg
    assert not os.path.exists(out)


# (write_pool arguments, ploidy, records, multi-allelic records the oracle writes)
POOL_CASES = {
    # the shrink loop, the called-allele set and the QS across blocks; column S (the reads of no sample) with reads
    "multi288": (dict(seed=62, depth=10.0 * 289, haplotypes=2, rg_samples=[f"P{k:04d}" for k in range(288)] + [None],
                      length=1500, site_rate=3e-4, multi_frac=0.5, n_contigs=1), 2, 92, 5),
    # the pool branch walking the scratch columns again per frequency hypothesis
    "pool272": (dict(seed=64, depth=12.0 * 272, haplotypes=4, rg_samples=[f"P{k:04d}" for k in range(272)],
                     length=1500, site_rate=3e-4, multi_frac=0.5, n_contigs=1), 4, 57, 5),
}


@pytest.mark.parametrize("case", sorted(POOL_CASES))
def test_wide_population_pool_data(tmp_path, case):
    from ngsepcore_amd import MultisampleVariantsDetector
    kw, ploidy, want, want_multi = POOL_CASES[case]
    fa, sam, bam = pool_data.write_pool(os.path.join(str(tmp_path), "pop"), **kw)
    o = os.path.join(str(tmp_path), "o.vcf")
    ngsep_oracle.run_mvd(fa, sam, o, 0.0, ploidy=ploidy)
    d = MultisampleVariantsDetector()
    d.setGenome(fa)
    d.setNormalPloidy(ploidy)
    d.setOutFilename(os.path.join(str(tmp_path), "g.vcf"))
    d.run([bam])
    _check(o, d.outFilename, want)
    multi = [l for l in open(o) if not l.startswith("#") and "," in l.split("\t")[4]]
    assert len(multi) >= want_multi
