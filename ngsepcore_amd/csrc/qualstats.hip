// qualstats.hip -- BasePairQualityStatisticsCalculator on gfx950 (alignments/BasePairQualityStatisticsCalculator.java:177-237).
//
// The reference walks every read base of every mapped record: a base that is one of ACGT and aligned (an M / = / X
// item, ReadAlignment.getReferencePositionAlignedRead :934-955) to a reference position holding one of ACGT counts
// in basesInRegion; a mismatch there adds one at its read position (counted from the 5' end: reversed on the negative
// strand), once more when the alignment is unique; an alignment with basesInRegion > 0 adds to the totals and to the
// by-length counts.  Integer counts only: exact in any order.
//
// Device input per batch: the records in BAM encoding -- the 4-bit SEQ bytes ("=ACMGRSVTWYHKDBN", high nibble first)
// and the reader's CIGAR words (NGSEP codes len * 8 + op, op: H0 D1 I2 M3 P4 N5 S6 X7: bit 1 = consumes the read,
// bit 0 = consumes the reference) as they are, and one 32-byte header per record.  The genome is resident as one code
// byte per position, all sequences back to back: the base's BAM nibble (A 1, C 2, G 4, T 8; case folded) or 0 for
// anything else, so a read nibble and a reference code compare directly.
//   KBQ k_readpos_stats : persistent workgroups of 4 wavefronts; a wavefront takes one record at a time, walks its
//                         CIGAR (wave-uniform state) and for every M / = / X item its 64 lanes take 64 consecutive read
//                         positions per step.  Mismatches add 1 | unique << 32 into LDS bins (read positions below
//                         kQsLdsBins; later positions go to the global arrays), the record's by-length and total
//                         updates are one lane's; a workgroup flushes its bins with global atomics once.
// Every index comes from the file, so every access is bounded: SEQ / CIGAR by the record's l_seq / n_cigar and by the
// batch buffers, the reference by the sequence's length (outside it a position does not count: getReferenceBase
// returning 0, ReferenceGenome.java:97-105) and by the genome array, a bin by the result arrays' capacity.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdint>
#include <algorithm>
#include <string>
#include <vector>
#include "engine.hpp"

namespace ngsep {

constexpr int kQsThreads = 256;                      // 4 wavefronts
constexpr int kQsLdsBins = 1024;                     // read positions (and read lengths) binned in LDS: 2 x 8 KB
constexpr int kQsSteps = 4;                          // 64-position steps of an item whose loads are in flight together

#define QS_TRY(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                   \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

struct QsDevice {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    int32_t n_cu = 256;
    // the genome's codes
    uint8_t* d_ref = nullptr;
    int64_t g_len = 0;
    // batch buffers: one pinned host block and its device twin, [headers | CIGAR words | SEQ bytes]
    uint8_t* h_stage = nullptr;
    uint8_t* d_stage = nullptr;
    size_t stage_cap = 0;
    size_t off_cig = 0, off_seq = 0;                 // the current batch's sections
    // results: 4 arrays of `cap` counts (mismatches, unique mismatches, alignments by length, unique by length), then
    // the totals (alignments, unique alignments, bases, unique bases)
    unsigned long long* d_out = nullptr;
    int64_t cap = 0;
    double kernel_ms = 0;                            // device time of the KBQ launches so far
};

__global__ void __launch_bounds__(kQsThreads)
k_readpos_stats(const QsRec* __restrict__ recs, int64_t n_rec, const uint8_t* __restrict__ seq, uint64_t seq_bytes,
                const uint32_t* __restrict__ cig, uint64_t cig_words, const uint8_t* __restrict__ ref, int64_t g_len,
                unsigned long long* __restrict__ out, int64_t cap) {
    __shared__ unsigned long long mis[kQsLdsBins];   // mismatches | unique mismatches << 32 per read position
    __shared__ unsigned long long byl[kQsLdsBins];   // alignments | unique alignments << 32 per read length - 1
    __shared__ unsigned long long tot[4];            // alignments, unique alignments, bases, unique bases
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < kQsLdsBins; k += kQsThreads) { mis[k] = 0ull; byl[k] = 0ull; }
    if (tid < 4) tot[tid] = 0ull;
    __syncthreads();
    const int64_t n_waves = (int64_t)gridDim.x * (kQsThreads / 64);
    const int64_t r0 = (int64_t)blockIdx.x * (kQsThreads / 64) + wave;
    QsRec hn = recs[r0 < n_rec ? r0 : 0];
    for (int64_t r = r0; r < n_rec; r += n_waves) {
        const QsRec h = hn;
        if (r + n_waves < n_rec) hn = recs[r + n_waves];     // the next record's header beside this one's loads
        const int64_t l_seq = h.l_seq;
        const uint32_t n_cig = h.ncf >> 2;
        const bool rev = (h.ncf & 1u) != 0;
        const unsigned long long uniq = (h.ncf >> 1) & 1u;
        const unsigned long long inc = 1ull | (uniq << 32);
        int64_t rp = 0, ro = 0;                      // read bases and reference positions before the item
        uint32_t counted = 0;                        // this lane's share of basesInRegion
        // (items past SEQ are never asked for; read positions past the items have no reference position)
        for (uint32_t k = 0; k < n_cig && rp < l_seq; k++) {
            const uint64_t ci = (uint64_t)h.cig_off + k;
            if (ci >= cig_words) break;
            const uint32_t w = cig[ci];
            const int64_t len = (int64_t)(w >> 3);
            const uint32_t op = w & 7u;
            if ((op & 3u) == 3u) {                   // M / = / X: read and reference
                const int64_t end = rp + len < l_seq ? rp + len : l_seq;
                // kQsSteps x 64 read positions per pass: every load of the pass is issued before the first compare
                // (a 150-base read is one pass: one load latency instead of three)
                for (int64_t j0 = rp; j0 < end; j0 += 64 * kQsSteps) {
                    uint32_t sb[kQsSteps], code[kQsSteps];
#pragma unroll
                    for (int u = 0; u < kQsSteps; u++) {
                        const int64_t j = j0 + u * 64 + lane;
                        const uint64_t si = (uint64_t)h.seq_off + (uint64_t)(j >> 1);
                        const int64_t d = ro + (j - rp);
                        const int64_t p = (int64_t)h.first + d;                 // 1-based position in its sequence
                        const int64_t gi = h.gfirst + d;
                        const bool in_read = j < end && si < seq_bytes;
                        const bool in_ref = in_read && p >= 1 && p <= (int64_t)h.seq_len && gi >= 0 && gi < g_len;
                        sb[u] = in_read ? (uint32_t)seq[si] : 0u;               // (no read base: nibble 0)
                        code[u] = in_ref ? (uint32_t)ref[gi] : 0u;              // (no reference base: code 0)
                    }
#pragma unroll
                    for (int u = 0; u < kQsSteps; u++) {
                        const int64_t j = j0 + u * 64 + lane;
                        const uint32_t nib = (sb[u] >> ((j & 1) ? 0 : 4)) & 15u;
                        // the read base and the reference base are each one of ACGT
                        if (nib == 0u || (nib & (nib - 1u)) != 0u || code[u] == 0u) continue;
                        counted++;
                        if (code[u] == nib) continue;
                        const int64_t b = rev ? l_seq - 1 - j : j;
                        if (b < kQsLdsBins) {
                            atomicAdd(&mis[b], inc);
                        } else if (b < cap) {
                            atomicAdd(&out[b], 1ull);
                            if (uniq) atomicAdd(&out[cap + b], 1ull);
                        }
                    }
                }
            }
            if (op & 2u) rp += len;
            if (op & 1u) ro += len;
        }
        unsigned long long nb = counted;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nb += __shfl_down(nb, o, 64);
        if (lane == 0 && nb > 0) {
            atomicAdd(&tot[0], 1ull);
            atomicAdd(&tot[2], nb);
            if (uniq) { atomicAdd(&tot[1], 1ull); atomicAdd(&tot[3], nb); }
            const int64_t b = l_seq - 1;
            if (b < kQsLdsBins) {
                atomicAdd(&byl[b], inc);
            } else if (b < cap) {
                atomicAdd(&out[2 * cap + b], 1ull);
                if (uniq) atomicAdd(&out[3 * cap + b], 1ull);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < kQsLdsBins && k < cap; k += kQsThreads) {
        const unsigned long long m = mis[k], l = byl[k];
        if (m & 0xffffffffull) atomicAdd(&out[k], m & 0xffffffffull);
        if (m >> 32) atomicAdd(&out[cap + k], m >> 32);
        if (l & 0xffffffffull) atomicAdd(&out[2 * cap + k], l & 0xffffffffull);
        if (l >> 32) atomicAdd(&out[3 * cap + k], l >> 32);
    }
    if (tid < 4 && tot[tid]) atomicAdd(&out[4 * cap + tid], tot[tid]);
}

QsDevice* qs_create(int ordinal, std::string& err) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        err = "no HIP device available (libngsep_amd requires an MI355X / gfx950 GPU)";
        return nullptr;
    }
    if (ordinal < 0 || ordinal >= n) { err = "device ordinal out of range"; return nullptr; }
    if (hipSetDevice(ordinal) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
    QsDevice* d = new QsDevice();
    d->ordinal = ordinal;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ordinal) == hipSuccess && prop.multiProcessorCount > 0) d->n_cu = prop.multiProcessorCount;
    }
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { err = "stream"; delete d; return nullptr; }
    for (auto& e : d->ev) (void)hipEventCreate(&e);
    return d;
}

void qs_destroy(QsDevice* d) {
    if (!d) return;
    (void)hipSetDevice(d->ordinal);
    (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->d_ref);
    (void)hipFree(d->d_stage);
    (void)hipFree(d->d_out);
    if (d->h_stage) pinned_free(d->h_stage);
    for (auto& e : d->ev) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(d->stream);
    delete d;
}

// the genome's codes: sequence k's characters at [start[k], start[k] + its length) of the device array
int qs_set_reference(QsDevice* d, const std::vector<std::string>& seqs, std::string& err) {
    QS_TRY(hipSetDevice(d->ordinal));
    QS_TRY(hipStreamSynchronize(d->stream));
    (void)hipFree(d->d_ref);
    d->d_ref = nullptr;
    int64_t total = 0;
    for (const auto& s : seqs) total += (int64_t)s.size();
    d->g_len = total;
    QS_TRY(hipMalloc(&d->d_ref, (size_t)std::max<int64_t>(total, 1)));
    uint8_t tab[256] = {};
    tab['A'] = tab['a'] = 1; tab['C'] = tab['c'] = 2; tab['G'] = tab['g'] = 4; tab['T'] = tab['t'] = 8;
    // through a pinned block of at most 64 MB (no copy's host side is pageable memory)
    const size_t blk = (size_t)std::min<int64_t>(std::max<int64_t>(total, 1), (int64_t)64 << 20);
    uint8_t* h = static_cast<uint8_t*>(pinned_alloc(blk));
    if (!h) { err = "pinned allocation failed"; return -1; }
    int rc = 0;
    int64_t at = 0;
    for (const auto& s : seqs) {
        for (size_t o = 0; o < s.size() && rc == 0; o += blk) {
            const size_t m = std::min(blk, s.size() - o);
            const char* src = s.data() + o;
            parallel_for((int64_t)m, 1 << 18, [&](int64_t lo, int64_t hi) {
                for (int64_t k = lo; k < hi; k++) h[k] = tab[(uint8_t)src[k]];
            });
            rc = dma_copy(d->d_ref + at + (int64_t)o, h, m, 0, d->stream, false, err, "qualstats.hip", __LINE__);
            if (rc == 0 && hipStreamSynchronize(d->stream) != hipSuccess) { err = "reference upload failed"; rc = -1; }
        }
        at += (int64_t)s.size();
        if (rc != 0) break;
    }
    pinned_free(h);
    return rc;
}

// pinned host buffers for a batch of n_rec records with n_cig CIGAR words and n_seq SEQ bytes in all (filled by the
// caller, then qs_run)
int qs_stage(QsDevice* d, int64_t n_rec, int64_t n_cig, int64_t n_seq, QsRec** rec, uint32_t** cig, uint8_t** seq, std::string& err) {
    QS_TRY(hipSetDevice(d->ordinal));
    const size_t b_rec = sizeof(QsRec) * (size_t)n_rec;
    const size_t b_cig = (sizeof(uint32_t) * (size_t)n_cig + 15) & ~(size_t)15;
    const size_t need = b_rec + b_cig + (size_t)n_seq + 16;
    if (need > d->stage_cap) {
        QS_TRY(hipStreamSynchronize(d->stream));
        size_t nc = d->stage_cap ? d->stage_cap : ((size_t)1 << 20);
        while (nc < need) nc *= 2;
        if (d->h_stage) pinned_free(d->h_stage);
        (void)hipFree(d->d_stage);
        d->h_stage = nullptr;
        d->d_stage = nullptr;
        d->stage_cap = 0;
        d->h_stage = static_cast<uint8_t*>(pinned_alloc(nc));
        if (!d->h_stage) { err = "pinned allocation failed"; return -1; }
        QS_TRY(hipMalloc(&d->d_stage, nc));
        d->stage_cap = nc;
    }
    d->off_cig = b_rec;
    d->off_seq = b_rec + b_cig;
    *rec = reinterpret_cast<QsRec*>(d->h_stage);
    *cig = reinterpret_cast<uint32_t*>(d->h_stage + d->off_cig);
    *seq = d->h_stage + d->off_seq;
    return 0;
}

// the result arrays hold at least `want` read positions (the counts so far are kept)
static int qs_grow(QsDevice* d, int64_t want, std::string& err) {
    if (want <= d->cap && d->d_out) return 0;
    int64_t nc = d->cap ? d->cap : 1024;
    while (nc < want) nc *= 2;
    unsigned long long* nb = nullptr;
    const size_t bytes = sizeof(unsigned long long) * (size_t)(4 * nc + 4);
    QS_TRY(hipMalloc(&nb, bytes));
    QS_TRY(hipMemsetAsync(nb, 0, bytes, d->stream));
    if (d->d_out) {
        for (int a = 0; a < 4; a++)
            QS_TRY(hipMemcpyAsync(nb + (size_t)a * (size_t)nc, d->d_out + (size_t)a * (size_t)d->cap,
                                  sizeof(unsigned long long) * (size_t)d->cap, hipMemcpyDeviceToDevice, d->stream));
        QS_TRY(hipMemcpyAsync(nb + (size_t)4 * (size_t)nc, d->d_out + (size_t)4 * (size_t)d->cap, sizeof(unsigned long long) * 4,
                              hipMemcpyDeviceToDevice, d->stream));
        QS_TRY(hipStreamSynchronize(d->stream));
        (void)hipFree(d->d_out);
    }
    d->d_out = nb;
    d->cap = nc;
    return 0;
}

// uploads the staged batch and runs KBQ over it; max_lseq: its longest read
int qs_run(QsDevice* d, int64_t n_rec, int64_t n_cig, int64_t n_seq, int64_t max_lseq, std::string& err) {
    QS_TRY(hipSetDevice(d->ordinal));
    if (!d->d_ref) { err = "no reference codes on the device"; return -1; }
    if (n_rec > kQsMaxRecords) { err = "too many records for one KBQ launch"; return -1; }
    if (qs_grow(d, std::max<int64_t>(max_lseq, 1), err) != 0) return -1;
    if (n_rec <= 0) return 0;
    const size_t bytes = d->off_seq + (size_t)n_seq;
    if (bytes > d->stage_cap) { err = "staged batch larger than its buffers"; return -1; }
    if (dma_copy(d->d_stage, d->h_stage, bytes, 0, d->stream, false, err, "qualstats.hip", __LINE__) != 0) return -1;
    int per_cu = 0;
    QS_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_readpos_stats, kQsThreads, 0));
    const int64_t want = (n_rec + kQsThreads / 64 - 1) / (kQsThreads / 64);
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)d->n_cu * std::max(1, per_cu)));
    hipExtLaunchKernelGGL(k_readpos_stats, dim3((unsigned)grid), dim3(kQsThreads), 0, d->stream, d->ev[0], d->ev[1], 0,
                          reinterpret_cast<const QsRec*>(d->d_stage), n_rec, d->d_stage + d->off_seq, (uint64_t)n_seq,
                          reinterpret_cast<const uint32_t*>(d->d_stage + d->off_cig), (uint64_t)n_cig, d->d_ref, d->g_len,
                          d->d_out, d->cap);
    QS_TRY(hipGetLastError());
    QS_TRY(hipStreamSynchronize(d->stream));
    float ms = 0.f;
    QS_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    d->kernel_ms += ms;
    return 0;
}

// the counts so far: out[a * n + i], a = 0..3 (mismatches, unique mismatches, by length, unique by length), i < n
// read positions, then the four totals at out[4 n ..]
int qs_fetch(QsDevice* d, int64_t n, uint64_t* out, std::string& err) {
    QS_TRY(hipSetDevice(d->ordinal));
    std::fill(out, out + 4 * n + 4, (uint64_t)0);
    if (!d->d_out) return 0;
    const int64_t m = std::min(n, d->cap);
    const size_t bytes = sizeof(unsigned long long) * (size_t)(4 * d->cap + 4);
    void* h = pinned_alloc(bytes);
    if (!h) { err = "pinned allocation failed"; return -1; }
    const int rc = dma_copy(h, d->d_out, bytes, 1, d->stream, false, err, "qualstats.hip", __LINE__);
    const hipError_t e = hipStreamSynchronize(d->stream);
    if (rc == 0 && e == hipSuccess) {
        const uint64_t* s = static_cast<const uint64_t*>(h);
        for (int a = 0; a < 4; a++) std::copy(s + (size_t)a * (size_t)d->cap, s + (size_t)a * (size_t)d->cap + m, out + (size_t)a * (size_t)n);
        std::copy(s + (size_t)4 * (size_t)d->cap, s + (size_t)4 * (size_t)d->cap + 4, out + (size_t)4 * (size_t)n);
    }
    pinned_free(h);
    if (rc != 0) return -1;
    QS_TRY(e);
    return 0;
}

int qs_clear(QsDevice* d, std::string& err) {
    QS_TRY(hipSetDevice(d->ordinal));
    if (d->d_out) {
        QS_TRY(hipMemsetAsync(d->d_out, 0, sizeof(unsigned long long) * (size_t)(4 * d->cap + 4), d->stream));
        QS_TRY(hipStreamSynchronize(d->stream));
    }
    d->kernel_ms = 0;
    return 0;
}

double qs_kernel_ms(const QsDevice* d) { return d ? d->kernel_ms : 0; }

}  // namespace ngsep
