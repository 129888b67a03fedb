"""Python restatement of the reference's BasePairQualStats command over SAM text (test infrastructure, never imported
by the product; independent of the oracle, which has no restatement of this command).

It follows alignments/BasePairQualityStatisticsCalculator.java line by line:
  * processFile :177-237 -- the reader with filterFlags = FLAG_READ_UNMAPPED alone (:179-180) and -minMQ (:181), the
    loop over the read's characters (:199-217), the per-alignment totals (:218-228);
  * printStatistics :248-258, makeCumulative :322-332, calculatePercentages :266-278;
and what processFile calls:
  * ReadAlignmentFileReader.loadAln / loadAlignment / isMultiple / isSameAlignment (io/ReadAlignmentFileReader.java:
    219-354): the drop of a record repeating the previous one, FLAG_MULTIPLE_ALN, the skip of a record whose
    loadAlignment throws (no CIGAR for a mapped read, read characters of another length than the CIGAR's);
  * ReadAlignment.setCigarString (:1222-1266, '=' read as M), getReferencePositionAlignedRead (:934-955),
    isUnique (:488), isNegativeStrand;
  * ReferenceGenome.getReferenceBase (genome/ReferenceGenome.java:97-105): 0 outside the sequence or for an unknown name;
  * DNASequence.isInAlphabeth (sequences/DNASequence.java:71-73): one of ACGT.

SEQ '*': loadAlignment never calls setReadCharacters (:260-262), getReadCharacters() is null and processFile :191
(read.length()) throws a NullPointerException that nothing catches: the reference's run dies.  The product skips such a
record (known divergence), and so does this restatement when skip_seq_star is set; otherwise it
raises like the reference.
"""
from __future__ import annotations

FLAG_READ_UNMAPPED = 0x4
FLAG_NEGATIVE = 0x10
FLAG_SECONDARY = 0x100
FLAG_MULTIPLE_ALN = 0x1000
DNA = "ACGT"

# ReadAlignment.java:60-69 operation codes; consumesReadBases / consumesReferenceBases
READ_OPS = set("IMSX=")
REF_OPS = set("DMNX=")


def load_fasta(path):
    """ReferenceGenome: name (to the first blank) -> bases, case kept"""
    seqs, name, buf = {}, None, []
    for l in open(path):
        l = l.rstrip("\r\n")
        if l.startswith(">"):
            if name is not None:
                seqs[name] = "".join(buf)
            name, buf = l[1:].split()[0], []
        elif name is not None:
            buf.append(l)
    if name is not None:
        seqs[name] = "".join(buf)
    return seqs


def parse_cigar(text):
    """[(op, length)] with '=' kept as its own letter (it behaves as M everywhere below)"""
    out, n = [], 0
    for ch in text:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            out.append((ch, n))
            n = 0
    return out


def reference_position_aligned_read(first, cigar, aligned_read_pos):
    """ReadAlignment.getReferencePositionAlignedRead (:934-955)"""
    current_ref_pos, current_aln_pos = first, 0
    for op, length in cigar:
        c_ref, c_read = op in REF_OPS, op in READ_OPS
        if c_ref and c_read:
            if aligned_read_pos < current_aln_pos:
                return -1
            if current_aln_pos + length > aligned_read_pos:
                return current_ref_pos + aligned_read_pos - current_aln_pos
        if c_ref:
            current_ref_pos += length
        if c_read:
            current_aln_pos += length
    return -1


def reference_base(genome, name, pos):
    """ReferenceGenome.getReferenceBase (:97-105): chr(0) for an unknown sequence or a position outside it"""
    s = genome.get(name)
    if s is None or pos < 1 or pos > len(s):
        return "\0"
    return s[pos - 1]


def is_multiple(flag, nh, mapq, min_mq):
    """ReadAlignmentFileReader.isMultiple (:284-291); nh: the NH attribute or None"""
    if flag & FLAG_SECONDARY:
        return True
    if nh is not None and nh > 1:
        return True
    if nh is not None and nh == 1:
        return False
    if mapq < min_mq:
        return True
    return False


def reader(sam_path, genome, min_mq):
    """The ReadAlignment objects processFile's iterator returns: (sequence name, first, cigar, flags, read characters)"""
    last = None
    for l in open(sam_path):
        if l.startswith("@"):
            continue
        f = l.rstrip("\n").split("\t")
        name, flag, rname, pos, mapq, cigar_text, seq = f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9]
        paired, fop = bool(flag & 1), bool(flag & 0x40)
        key = (name, pos, paired, fop if paired else None)
        if last is not None and key == last:                     # isSameAlignment (:292-306, :337)
            continue
        last = key
        tags = dict((t[:2], t[5:]) for t in f[11:])
        nh = int(tags["NH"]) if "NH" in tags else None
        flags = flag + (FLAG_MULTIPLE_ALN if is_multiple(flag, nh, mapq, min_mq) else 0)    # (:229-230)
        if flags & FLAG_READ_UNMAPPED:                           # filterFlags (:350)
            continue
        if rname not in genome:                                  # (a mapped record names a header sequence)
            continue
        if cigar_text == "*":                                    # setCigarString(null) on a mapped read throws: skipped (:341-347)
            continue
        cigar = parse_cigar(cigar_text)
        read_len = sum(n for op, n in cigar if op in READ_OPS)
        chars = None if seq == "*" else seq
        if chars is not None and len(chars) != read_len:         # setReadCharacters throws (ReadAlignment.java:550): skipped
            continue
        yield rname, pos, cigar, flags, chars


class QualStats:
    """The calculator's model attributes (:63-70)"""

    def __init__(self):
        self.mismatches, self.mismatches_unique = [], []
        self.alns_by_length, self.unique_by_length = [], []
        self.total_alignments = self.total_bases = self.reads_unique = self.bases_unique = 0

    def process_file(self, sam_path, genome, min_mq=20, skip_seq_star=True):
        """processFile (:177-237)"""
        for seq_name, first, cigar, flags, read in reader(sam_path, genome, min_mq):
            if read is None:
                if skip_seq_star:
                    continue
                raise TypeError("read.length() on null read characters (:191)")
            reverse = bool(flags & FLAG_NEGATIVE)
            unique_aln = not flags & FLAG_MULTIPLE_ALN
            bases_in_region = 0
            read_length = len(read)
            while read_length > len(self.mismatches):                       # :192-198
                for lst in (self.mismatches, self.mismatches_unique, self.alns_by_length, self.unique_by_length):
                    lst.append(0)
            for j in range(len(read)):                                      # :199-217
                base_read = read[j].upper()
                if base_read in DNA:
                    pos = reference_position_aligned_read(first, cigar, j)
                    if pos > 0:
                        base_ref = reference_base(genome, seq_name, pos).upper()
                        if base_ref != "\0" and base_ref in DNA:
                            bases_in_region += 1
                            if base_read != base_ref:
                                pos_stats = len(read) - 1 - j if reverse else j
                                self.mismatches[pos_stats] += 1
                                if unique_aln:
                                    self.mismatches_unique[pos_stats] += 1
            if bases_in_region > 0:                                         # :218-228
                self.total_alignments += 1
                self.total_bases += bases_in_region
                self.alns_by_length[read_length - 1] += 1
                if unique_aln:
                    self.reads_unique += 1
                    self.bases_unique += bases_in_region
                    self.unique_by_length[read_length - 1] += 1

    @staticmethod
    def make_cumulative(data):
        """makeCumulative (:322-332): answer[i] = the sum of data[i..n) (its double loop as one backward pass)"""
        out, t = [0] * len(data), 0
        for i in range(len(data) - 1, -1, -1):
            t += data[i]
            out[i] = t
        return out

    def report(self):
        """printStatistics (:248-258)"""
        ca, cu = self.make_cumulative(self.alns_by_length), self.make_cumulative(self.unique_by_length)
        lines = [f"{i + 1}\t{self.mismatches[i]}\t{self.mismatches_unique[i]}\t{ca[i]}\t{cu[i]}"
                 for i in range(len(self.mismatches))]
        lines += ["", f"Alignments\t{self.total_alignments}\t{self.reads_unique}",
                  f"Bases\t{self.total_bases}\t{self.bases_unique}"]
        return "\n".join(lines) + "\n"

    def percentages(self, unique_alignments):
        """calculatePercentages (:266-278), Java double division (0 / 0 = NaN, x / 0 = Infinity)"""
        m = self.mismatches_unique if unique_alignments else self.mismatches
        cum = self.make_cumulative(self.unique_by_length if unique_alignments else self.alns_by_length)
        out = []
        for a, b in zip(m, cum):
            x = 100.0 * a
            out.append(x / b if b else (float("nan") if x == 0 else float("inf")))
        return out


def run(sam_paths, fasta_path, min_mq=20, skip_seq_star=True):
    """run() (:146-160): init, every file, the statistics"""
    genome = load_fasta(fasta_path)
    st = QualStats()
    for p in sam_paths:
        st.process_file(p, genome, min_mq, skip_seq_star)
    return st
