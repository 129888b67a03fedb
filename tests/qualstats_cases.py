"""Seeded inputs of the BasePairQualStats tests (test infrastructure): a hand-made case whose report is derived by hand
from alignments/BasePairQualityStatisticsCalculator.java:177-258, reads whose lengths straddle the kernel's 64-lane
steps with every CIGAR shape and reader corner case, and a 50,000-base read.  SAM text plus FASTA; the device path
reads the same records as BAM (pysynth.sam_to_bam).  Qualities are '*' throughout: the command never reads them."""
from __future__ import annotations

import os

import numpy as np

BASES = "ACGT"


def _write(d, stem, contigs, lines):
    fa, sam = os.path.join(str(d), stem + ".fa"), os.path.join(str(d), stem + ".sam")
    with open(fa, "w") as f:
        for name, s in contigs:
            f.write(f">{name}\n")
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.6\tSO:coordinate\n")
        for name, s in contigs:
            f.write(f"@SQ\tSN:{name}\tLN:{len(s)}\n")
        f.writelines(lines)
    return fa, sam


def _line(name, flag, contig, pos, mapq, cigar, seq, tags=()):
    return "\t".join([name, str(flag), contig, str(pos), str(mapq), cigar, "*", "0", "0", seq, "*", *tags]) + "\n"


# ---- the hand-made case ---------------------------------------------------------------------------------------------
# c1: base at 1-based p = "ACGT"[(p - 1) % 4].
#   r1 8M at 1 ACGTACGA: mismatch at j = 7; unique; 8 bases
#   r3 4M at 1 NCGT, MAPQ 5: the N is skipped (3 bases); not unique
#   r4 secondary 4M at 3 GTAA: reference GTAC, mismatch at j = 3; kept, not unique; 4 bases
#   r2 reverse 2S4M2I2M at 5 TTACGAGGAC: j 2..5 ACGA on ACGT -> mismatch at j = 5 = position 10 - 1 - 5 = 4; j 8, 9 AC
#      on AC; unique; 6 bases
#   r6 3M1D3M at 11 GTAGTC, MAPQ 0 but NH 1: unique; GTA on GTA, the deletion skips 14, GTC on GTA (15..17) -> j = 5; 6 bases
#   r5 unmapped: filtered
HAND_REPORT = ("1\t0\t0\t5\t3\n2\t0\t0\t5\t3\n3\t0\t0\t5\t3\n4\t1\t0\t5\t3\n5\t1\t1\t3\t3\n6\t1\t1\t3\t3\n7\t0\t0\t2\t2\n"
               "8\t1\t1\t2\t2\n9\t0\t0\t1\t1\n10\t0\t0\t1\t1\n\nAlignments\t5\t3\nBases\t27\t20\n")


def hand_case(d):
    ref = "".join(BASES[p % 4] for p in range(40))
    lines = [_line("r1", 0, "c1", 1, 60, "8M", "ACGTACGA"),
             _line("r3", 0, "c1", 1, 5, "4M", "NCGT"),
             _line("r4", 256, "c1", 3, 60, "4M", "GTAA"),
             _line("r2", 16, "c1", 5, 60, "2S4M2I2M", "TTACGAGGAC"),
             _line("r6", 0, "c1", 11, 0, "3M1D3M", "GTAGTC", ("NH:i:1",)),
             "\t".join(["r5", "4", "*", "0", "0", "*", "*", "0", "0", "ACGTACGT", "*"]) + "\n"]
    return _write(d, "hand", [("c1", ref)], lines)


# ---- reads around the 64-lane steps ---------------------------------------------------------------------------------
def _rand(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, size=n))


def _read_from(rng, ref, pos, ops, mut=0.05, n_rate=0.02, lower=0.03):
    """SEQ of a read at 1-based pos with items ops: reference bases (random where the reference has none), a few
    substitutions, N bases and lower-case characters"""
    out, rp = [], pos - 1
    for op, n in ops:
        if op in "M=X":
            for k in range(n):
                b = ref[rp + k].upper() if rp + k < len(ref) else "?"
                if b not in BASES:
                    b = BASES[int(rng.integers(4))]
                if rng.random() < mut:
                    b = BASES[(BASES.index(b) + 1 + int(rng.integers(3))) % 4]
                if rng.random() < n_rate:
                    b = "N"
                out.append(b.lower() if rng.random() < lower else b)
            rp += n
        elif op in "IS":
            out.extend(_rand(rng, n))
        elif op in "DN":
            rp += n
    return "".join(out)


def _eqx(ops, seq, ref, pos):
    out, rp, qp = [], pos - 1, 0
    for op, n in ops:
        if op == "M":
            for k in range(n):
                o = "=" if rp + k < len(ref) and seq[qp + k].upper() == ref[rp + k].upper() else "X"
                if out and out[-1][0] == o:
                    out[-1] = (o, out[-1][1] + 1)
                else:
                    out.append((o, 1))
        else:
            out.append((op, n))
        if op in "MDN":
            rp += n
        if op in "MIS":
            qp += n
    return out


def _cig(ops):
    return "".join(f"{n}{o}" for o, n in ops)


def _span(ops):
    return sum(n for o, n in ops if o in "MDN=X")


def lane_shapes(d, seed=1, length=3000, depth=6.0):
    """One contig with N and lower-case stretches; read lengths 1, 63, 64, 65, 128, 129 on both strands with soft and
    hard clips, I / D / N / = / X / P items, N bases, MAPQ on both sides of 20 and 30, NH absent / 1 / 2, secondary and
    supplementary records, a record repeated verbatim, a read of 141 CIGAR items, a read whose last M item runs past the
    contig's end, an unmapped record"""
    rng = np.random.default_rng(seed)
    s = list(_rand(rng, length))
    for a, b in ((100, 160), (1500, 1510), (2900, 2930)):
        s[a:b] = "N" * (b - a)
    for a, b in ((400, 700), (2000, 2100)):
        s[a:b] = [c.lower() for c in s[a:b]]
    ref = "".join(s)
    recs, bases, k = [], 0, 0
    lengths = (1, 63, 64, 65, 128, 129)
    styles = ("M", "S", "H", "I", "D", "N", "EQX", "P")
    while bases < depth * length:
        L = lengths[k % len(lengths)]
        style = styles[(k // len(lengths)) % len(styles)] if L >= 8 else ("M", "H", "EQX")[k % 3]
        k += 1
        a = int(rng.integers(1, L - 2)) if L >= 8 else 0
        if style == "S":
            b = int(rng.integers(1, L - a))
            ops = [("S", a), ("M", L - a - b), ("S", b)] if L - a - b > 0 else [("S", a), ("M", L - a)]
        elif style == "H":
            ops = [("H", 5), ("M", L), ("H", 3)]
        elif style == "I":
            kk = int(rng.integers(1, min(4, L - a)))
            ops = [("M", a), ("I", kk), ("M", L - a - kk)] if L - a - kk > 0 else [("M", a), ("I", L - a)]
        elif style == "D":
            ops = [("M", a), ("D", int(rng.integers(1, 5))), ("M", L - a)]
        elif style == "N":
            ops = [("M", a), ("N", int(rng.integers(100, 300))), ("M", L - a)]
        elif style == "P":
            ops = [("M", a), ("P", 1), ("M", L - a)]
        else:
            ops = [("M", L)]
        pos = int(rng.integers(1, length - _span(ops)))
        seq = _read_from(rng, ref, pos, ops)
        if style == "EQX":
            ops = _eqx(ops, seq, ref, pos)
        flag = (16 if rng.random() < 0.5 else 0) | (0x100 if rng.random() < 0.06 else 0) | (0x800 if rng.random() < 0.06 else 0) | \
               (0x400 if rng.random() < 0.03 else 0)
        mapq = int(rng.choice([0, 10, 19, 20, 25, 29, 30, 60]))
        nh = int(rng.integers(4))
        tags = () if nh == 0 else (f"NH:i:{nh}",)
        recs.append((pos, len(recs), _line(f"q{k}", flag, "c1", pos, mapq, _cig(ops), seq, tags)))
        bases += L
    # 141 items: (1M 1D) x 35, (1M 1I) x 35, 24M = 129 read bases
    ops = [("M", 1), ("D", 1)] * 35 + [("M", 1), ("I", 1)] * 35 + [("M", 24)]
    recs.append((777, len(recs), _line("many_items", 16, "c1", 777, 60, _cig(ops), _read_from(rng, ref, 777, ops))))
    # the last M item runs 78 positions past the contig's end
    pos = length - 49
    recs.append((pos, len(recs), _line("past_end", 0, "c1", pos, 60, "128M", _read_from(rng, ref, pos, [("M", 128)]))))
    recs.sort(key=lambda t: (t[0], t[1]))
    lines = []
    for i, (_, _, l) in enumerate(recs):
        lines.append(l)
        if i % 37 == 5:
            lines.append(l)                               # the same name and start twice in a row (isSameAlignment)
    lines.append("\t".join(["un", "4", "*", "0", "0", "*", "*", "0", "0", "ACGTACGTAC", "*"]) + "\n")
    return _write(d, f"lanes{seed}", [("c1", ref)], lines)


# ---- a 50,000-base read ---------------------------------------------------------------------------------------------
def long_read(d, seed=2, length=60000, long_len=50000):
    """100-base reads before and after one long_len-base read (reverse strand, an insertion and a deletion inside) with
    mismatches near both of its ends"""
    rng = np.random.default_rng(seed)
    ref = _rand(rng, length)
    recs = []
    for i, pos in enumerate((5, 300, 700, 2000, length - 8000, length - 1000)):
        recs.append((pos, _line(f"s{i}", 16 * (i & 1), "c1", pos, 60, "100M", _read_from(rng, ref, pos, [("M", 100)], n_rate=0.0))))
    a, b = long_len * 2 // 5, long_len // 5
    ops = [("M", a), ("I", 3), ("M", b), ("D", 7), ("M", long_len - a - 3 - b)]
    seq = list(_read_from(rng, ref, 1001, ops, mut=0.0, n_rate=0.0, lower=0.0))
    for j in (0, 3, 1500, long_len - 10, long_len - 1):
        seq[j] = BASES[(BASES.index(seq[j]) + 1) % 4]
    recs.append((1001, _line("long", 16, "c1", 1001, 60, _cig(ops), "".join(seq))))
    recs.sort(key=lambda t: t[0])
    return _write(d, f"long{seed}", [("c1", ref)], [l for _, l in recs])
