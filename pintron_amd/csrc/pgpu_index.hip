// Genomic index resident in HBM -- the sequence (1 B/base), its suffix array and LCP array, which stand in for the
// reference's augmented suffix tree:
//   lst_stree_new (stree_src/lst_stree.c:816) and stree_preprocess (src/aug_suffix_tree.c:247).
// What reads it: the pairing kernels (pgpu_pairing_plan.hip, through PairIndexView), the suffix-array form of the longest
// common factor (pgpu_dp_kernels.hip, through LcfIndexView) and the queries on the index (pgpu_query_call.h).
//
// Index build: prefix doubling on the device; the device-wide sorts and scans are rocPRIM
// (one-off per gene, not a hot path).
#include <algorithm>
#include <unistd.h>
#include <sys/stat.h>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>   // index construction only (one-off per gene)
#include <rocprim/device/device_scan.hpp>

#include "pgpu_index.h"

// The first KTAB (pgpu_index.h) characters of a pattern position select the suffix-array interval of that
// KTAB-mer from a table (2 x 4^KTAB x 4 B = 512 KB, L2-resident) instead of ~2 x 17 bisection
// steps over the whole array; the bisection continues inside that interval (a handful of
// suffixes) from character KTAB on.  Only upper-case ACGT k-mers are tabulated (kmer_code, pgpu_index.h).

struct pgpu_index {
  uint8_t* d_gen = nullptr;
  uint32_t* d_sa = nullptr;
  uint32_t* d_lcp = nullptr;      // n+1 entries; lcp[0] = lcp[n] = 0
  uint32_t* d_klo = nullptr;      // [code] -> first suffix-array index of the k-mer (klo == khi: absent)
  uint32_t* d_khi = nullptr;
  // preprocess_text (src/aug_suffix_tree.c:68-120): key of a character = its rank among the distinct
  // characters of the genomic sequence, `sigma` (their number) for characters that do not occur
  uint8_t* d_key = nullptr;          // 256 entries
  uint32_t sigma = 0;
  size_t len = 0;
  // derived tables for the suffix-array longest-common-factor search (LcfIndexView, pgpu_index.h); made
  // after every build and load, not kept in the index file
  uint32_t* d_focc = nullptr;
  uint32_t* d_rmq = nullptr;
  uint32_t rmq_levels = 0, first_bad = 0;
  // the sequence at 2 bits per base (16 bases per word) + 1 flag bit per base for "not an upper-case A, C, G, T"
  // (32 per word): what the pairing kernels compare on (PackedSeq); the bytes stay for the flagged stretches
  uint32_t* d_code = nullptr;
  uint32_t* d_bad = nullptr;
  // made on first use by whoever needs them (pgpu_index.h); nothing is built or allocated for them here
  mutable pgpu_index_lazy lazy;
};

LcfIndexView pgpu_index_lcf_view(const pgpu_index* idx) {
  LcfIndexView v{};
  if (idx) { v.T = idx->d_gen; v.sa = idx->d_sa; v.klo = idx->d_klo; v.khi = idx->d_khi; v.focc = idx->d_focc; v.rmq = idx->d_rmq;
             v.n = (uint32_t)idx->len; v.levels = idx->rmq_levels; v.first_bad = idx->first_bad; }
  return v;
}

PairIndexView pgpu_index_pair_view(const pgpu_index* idx) {
  return PairIndexView{idx->d_gen, (uint32_t)idx->len, idx->d_sa, idx->d_lcp, idx->d_klo, idx->d_khi, idx->d_key, idx->sigma,
                       idx->d_code, idx->d_bad};
}

const uint8_t* pgpu_index_genomic(const pgpu_index* idx) { return idx->d_gen; }
size_t pgpu_index_length(const pgpu_index* idx) { return idx->len; }
pgpu_index_lazy* pgpu_index_lazy_slot(const pgpu_index* idx) { return &idx->lazy; }

namespace {

// ---------------------------------------------------------------------------------------------
// suffix array by prefix doubling
// ---------------------------------------------------------------------------------------------
__global__ void sa_init_kernel(const uint8_t* __restrict__ T, uint32_t n, uint32_t* rank, uint32_t* sa) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { rank[i] = (uint32_t)T[i] + 1u; sa[i] = i; }
}

__global__ void sa_keys_kernel(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ sa,
                               uint32_t n, uint32_t h, unsigned long long* keys) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = sa[k];
  const uint32_t r2 = (i + h < n) ? rank[i + h] : 0u;          // past the end sorts first ('$')
  keys[k] = ((unsigned long long)rank[i] << 32) | r2;
}

__global__ void sa_flags_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* flags) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) flags[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1u : 0u;
}

__global__ void sa_rerank_kernel(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ newrank_sorted,
                                 uint32_t n, uint32_t* rank) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) rank[sa[k]] = newrank_sorted[k];
}

// LCP of neighbouring suffixes from the rank arrays the prefix doubling went through: ranks[r] orders
// the suffixes by their first 2^r characters (the end of the text sorting first), so two suffixes
// share 2^r more characters exactly when their ranks[r] agree; descending r adds up the exact LCP
// in ~log n steps per pair, however repetitive the sequence is (a character-by-character scan is
// quadratic on a long exact repeat).
__global__ void lcp_from_ranks_kernel(const uint32_t* const* __restrict__ ranks, int n_rounds,
                                      const uint32_t* __restrict__ sa, uint32_t n, uint32_t* __restrict__ lcp) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n) return;
  if (k == 0 || k == n) { lcp[k] = 0; return; }
  const uint32_t a = sa[k - 1], b = sa[k];
  uint32_t l = 0;
  for (int r = n_rounds - 1; r >= 0; --r) {
    if (a + l < n && b + l < n && ranks[r][a + l] == ranks[r][b + l]) l += 1u << r;
  }
  lcp[k] = l;
}

// suffixes sharing a KTAB-mer are contiguous in the suffix array: mark where each run starts/ends
__global__ void kmer_table_kernel(const uint8_t* __restrict__ T, uint32_t n, const uint32_t* __restrict__ sa,
                                  uint32_t* __restrict__ klo, uint32_t* __restrict__ khi) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int c = kmer_code(T + sa[k], n - sa[k]);
  if (c < 0) return;
  const int prev = k > 0 ? kmer_code(T + sa[k - 1], n - sa[k - 1]) : -1;
  const int next = k + 1 < n ? kmer_code(T + sa[k + 1], n - sa[k + 1]) : -1;
  if (prev != c) klo[c] = k;
  if (next != c) khi[c] = k + 1;
}

// first occurrence of every l-mer (l = 1..8) that starts at t: tables zero-based at (4^l - 4) / 3
__global__ void first_occ_kernel(const uint8_t* __restrict__ T, uint32_t n, uint32_t* __restrict__ focc) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t code = 0, off = 0, width = 4;
  for (uint32_t l = 1; l <= 8 && t + l <= n; ++l) {
    const int b = kmer_base(T[t + l - 1]);
    if (b < 0) break;
    code = code * 4 + (uint32_t)b;
    // (a first occurrence lies early in the sequence: nearly every thread sees a smaller value already there and
    // skips the atomic -- a million atomics on the four entries of l = 1 took 8 ms on a 1 Mb sequence)
    if (t < focc[off + code]) atomicMin(&focc[off + code], t);
    off += width; width *= 4;
  }
}
// one level of the sparse table: out[k] = min(in[k], in[k + half]) for k + 2 * half <= n
__global__ void rmq_level_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t half, uint32_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k + 2 * half <= n) out[k] = min(in[k], in[k + half]);
}

// the sequence at 2 bits per base and a flag bit per base that is not an upper-case A, C, G or T: one thread per flag word
// (32 bases); what the pairing kernels compare on (PackedSeq, pgpu_pairing_plan.hip)
__global__ void pack2_kernel(const uint8_t* __restrict__ src, unsigned long long n, uint32_t* __restrict__ code,
                             uint32_t* __restrict__ bad, unsigned long long n_bad_words) {
  const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;    // one flag word = 32 bases
  if (w >= n_bad_words) return;
  uint32_t c0 = 0, c1 = 0, b = 0;
  for (uint32_t k = 0; k < 32; ++k) {
    const unsigned long long p = w * 32 + k;
    const int x = p < n ? kmer_base(src[p]) : -1;
    if (x < 0) b |= 1u << k;
    else if (k < 16) c0 |= (uint32_t)x << (2 * k);
    else c1 |= (uint32_t)x << (2 * (k - 16));
  }
  code[2 * w] = c0; code[2 * w + 1] = c1; bad[w] = b;
}

template <class T> hipError_t dmalloc(T** p, size_t count) {
  return hipMalloc((void**)p, (count ? count : 1) * sizeof(T));
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C-ABI: index
// ---------------------------------------------------------------------------------------------
// alphabet keys of the genomic sequence (host), uploaded with the index
static hipError_t upload_keys(pgpu_index* idx, const char* genomic, size_t len, hipStream_t st) {
  bool seen[256] = {false};
  for (size_t i = 0; i < len; ++i) seen[(unsigned char)genomic[i]] = true;
  uint8_t key[256];
  uint32_t sigma = 0;
  for (int c = 0; c < 256; ++c) if (seen[c]) key[c] = (uint8_t)sigma++;
  for (int c = 0; c < 256; ++c) if (!seen[c]) key[c] = (uint8_t)(sigma > 255 ? 255 : sigma);
  idx->sigma = sigma;
  hipError_t e = hipMalloc((void**)&idx->d_key, 256);
  if (e != hipSuccess) return e;
  e = hipMemcpyAsync(idx->d_key, key, 256, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  return hipStreamSynchronize(st);           // `key` is a local
}

hipError_t pack_sequence(const uint8_t* src, size_t n, uint32_t* code, uint32_t* bad, hipStream_t st) {
  const size_t bad_words = (n + 31) / 32;
  hipError_t e = hipMemsetAsync(code + 2 * bad_words, 0, 4 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(bad + bad_words, 0xFF, 4 * sizeof(uint32_t), st);
  if (e != hipSuccess || bad_words == 0) return e;
  hipLaunchKernelGGL(pack2_kernel, dim3((unsigned)((bad_words + 255) / 256)), dim3(256), 0, st, src, (unsigned long long)n, code, bad,
                     (unsigned long long)bad_words);
  return hipGetLastError();
}

// tables derived from (sequence, suffix array): see LcfIndexView
static hipError_t build_lcf_tables(pgpu_index* idx, const char* genomic, hipStream_t st) {
  const uint32_t n = (uint32_t)idx->len;
  {
    const size_t bad_words = ((size_t)n + 31) / 32;
    hipError_t pe = hipMalloc((void**)&idx->d_code, (2 * bad_words + 4) * sizeof(uint32_t));
    if (pe != hipSuccess) return pe;
    pe = hipMalloc((void**)&idx->d_bad, (bad_words + 4) * sizeof(uint32_t));
    if (pe != hipSuccess) return pe;
    pe = pack_sequence(idx->d_gen, n, idx->d_code, idx->d_bad, st);
    if (pe != hipSuccess) return pe;
  }
  uint32_t fb = n;
  for (uint32_t i = 0; i < n; ++i) { const char c = genomic[i]; if (c != 'A' && c != 'C' && c != 'G' && c != 'T') { fb = i; break; } }
  idx->first_bad = fb;
  // The tables of the suffix-array LCF are optional: floor(log2 n) x n x 4 B of range minima is 14 MB for a 200 kb
  // gene but 10 GB for 100 Mb.  Without them (a sequence beyond PGPU_LCF_SA_MAX_BASES -- default 2^26 --, or no
  // memory) every LCF job takes lcf_kernel: pgpu_dp_plan_create_parts looks at d_focc / d_rmq.
  {
    const char* mx = getenv("PGPU_LCF_SA_MAX_BASES");
    const unsigned long long max_bases = mx && atoll(mx) > 0 ? (unsigned long long)atoll(mx) : (1ull << 26);
    if (n > max_bases) return hipSuccess;
  }
  hipError_t e = hipMalloc((void**)&idx->d_focc, LCF_FOCC_ENTRIES * sizeof(uint32_t));
  if (e != hipSuccess) { idx->d_focc = nullptr; (void)hipGetLastError(); return hipSuccess; }
  e = hipMemsetAsync(idx->d_focc, 0xFF, LCF_FOCC_ENTRIES * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  uint32_t levels = 0;
  while (n >= 2 && (2u << levels) <= n) ++levels;              // levels j = 1..levels with 2^j <= n
  idx->rmq_levels = levels;
  e = hipMalloc((void**)&idx->d_rmq, ((size_t)(levels ? levels : 1) * (n ? n : 1)) * sizeof(uint32_t));
  if (e != hipSuccess) {                                       // no room for the range minima: the matrix kernel serves
    idx->d_rmq = nullptr; idx->rmq_levels = 0; (void)hipGetLastError();
    hipFree(idx->d_focc); idx->d_focc = nullptr;
    return hipSuccess;
  }
  if (n == 0) return hipSuccess;
  const dim3 blk(256), grd((n + 255) / 256);
  hipLaunchKernelGGL(first_occ_kernel, grd, blk, 0, st, idx->d_gen, n, idx->d_focc);
  for (uint32_t j = 1; j <= levels; ++j)
    hipLaunchKernelGGL(rmq_level_kernel, grd, blk, 0, st, j == 1 ? idx->d_sa : idx->d_rmq + (size_t)(j - 2) * n, n, 1u << (j - 1),
                       idx->d_rmq + (size_t)(j - 1) * n);
  return hipGetLastError();
}

#define TRY_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) { rc = pgpu_ctx_fail(ctx, e_ == hipErrorOutOfMemory ? PGPU_ENOMEM : PGPU_EDEVICE, \
                                               hipGetErrorString(e_)); goto done; }          \
  } while (0)

static double idx_now_ms() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

extern "C" int pgpu_index_build(pgpu_ctx* ctx, const char* genomic, size_t len, pgpu_index** out) {
  if (!ctx || !out || (len && !genomic)) return PGPU_EINVAL;
  const bool timing = getenv("PGPU_INDEX_TIMING") != nullptr;      // phases of the construction, to stderr
  double t_mark = idx_now_ms();
  int n_rounds = 0;
  auto mark = [&](const char* what, hipStream_t s) {
    if (!timing) return;
    hipStreamSynchronize(s);
    const double t = idx_now_ms();
    fprintf(stderr, "* index build: %-28s %7.2f ms\n", what, t - t_mark);
    t_mark = t;
  };
  *out = nullptr;
  if (len >= (1u << 28)) return pgpu_ctx_fail(ctx, PGPU_ERANGE, "genomic longer than 2^28");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  pgpu_index* idx = new (std::nothrow) pgpu_index();
  if (!idx) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory");
  idx->len = len;
  hipStream_t st = pgpu_ctx_stream(ctx);
  const uint32_t n = (uint32_t)len;
  int rc = PGPU_OK;
  uint32_t *rank = nullptr, *sa2 = nullptr, *flags = nullptr, *newrank = nullptr;
  std::vector<uint32_t*> round_ranks;        // rank arrays by 2^r-character prefixes, r = 0, 1, ...
  const uint32_t** d_round_ptrs = nullptr;
  unsigned long long *keys = nullptr, *keys2 = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  const dim3 blk(256), grd((n + 255) / 256 + 1);

  TRY_HIP(hipMalloc((void**)&idx->d_gen, len + 64));
  TRY_HIP(hipMemsetAsync(idx->d_gen, 0, len + 64, st));
  if (len) TRY_HIP(hipMemcpyAsync(idx->d_gen, genomic, len, hipMemcpyHostToDevice, st));
  TRY_HIP(upload_keys(idx, genomic, len, st));
  TRY_HIP(dmalloc(&idx->d_sa, n + 1));
  TRY_HIP(dmalloc(&idx->d_lcp, n + 2));
  if (n > 0) {
    TRY_HIP(dmalloc(&rank, n)); TRY_HIP(dmalloc(&sa2, n)); TRY_HIP(dmalloc(&flags, n));
    TRY_HIP(dmalloc(&newrank, n)); TRY_HIP(dmalloc(&keys, n)); TRY_HIP(dmalloc(&keys2, n));
    {
      size_t b1 = 0, b2 = 0;
      TRY_HIP(rocprim::radix_sort_pairs(nullptr, b1, keys, keys2, idx->d_sa, sa2, n, 0, 64, st));
      TRY_HIP(rocprim::inclusive_scan(nullptr, b2, flags, newrank, n, rocprim::plus<uint32_t>(), st));
      tmp_bytes = b1 > b2 ? b1 : b2;
      TRY_HIP(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
    }
    hipLaunchKernelGGL(sa_init_kernel, grd, blk, 0, st, idx->d_gen, n, rank, idx->d_sa);
    mark("allocations + upload", st);
    for (uint32_t h = 0;; h = h ? h * 2 : 1) {
      ++n_rounds;
      // h == 0: sort by the first character alone (key low half = 0 because i+0 < n gives rank[i]
      // again -- harmless duplicate), afterwards by (rank of 2^k prefix, rank of the next 2^k)
      hipLaunchKernelGGL(sa_keys_kernel, grd, blk, 0, st, rank, idx->d_sa, n, h ? h : n, keys);
      size_t b = tmp_bytes;
      TRY_HIP(rocprim::radix_sort_pairs(tmp, b, keys, keys2, idx->d_sa, sa2, n, 0, 64, st));
      hipLaunchKernelGGL(sa_flags_kernel, grd, blk, 0, st, keys2, n, flags);
      b = tmp_bytes;
      TRY_HIP(rocprim::inclusive_scan(tmp, b, flags, newrank, n, rocprim::plus<uint32_t>(), st));
      hipLaunchKernelGGL(sa_rerank_kernel, grd, blk, 0, st, sa2, newrank, n, rank);
      {                                        // this round ranked by the first max(1, 2h) characters
        uint32_t* keep = nullptr;
        TRY_HIP(dmalloc(&keep, n));
        round_ranks.push_back(keep);
        TRY_HIP(hipMemcpyAsync(keep, rank, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      }
      TRY_HIP(hipMemcpyAsync(idx->d_sa, sa2, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      uint32_t distinct = 0;
      TRY_HIP(hipMemcpyAsync(&distinct, newrank + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      TRY_HIP(hipStreamSynchronize(st));
      if (distinct == n) break;
      if (h >= n) { rc = pgpu_ctx_fail(ctx, PGPU_EDEVICE, "suffix array construction did not converge"); goto done; }
    }
  }
  if (timing) fprintf(stderr, "* index build: %d sort rounds\n", n_rounds);
  mark("suffix array (sort rounds)", st);
  {
    // round 0 ranked by 1 character (h == 0), round j >= 1 by 2^j characters: ranks[r] <-> 2^r
    const int nr = (int)round_ranks.size();
    TRY_HIP(hipMalloc((void**)&d_round_ptrs, (nr ? nr : 1) * sizeof(uint32_t*)));
    if (nr) TRY_HIP(hipMemcpyAsync(d_round_ptrs, round_ranks.data(), nr * sizeof(uint32_t*), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lcp_from_ranks_kernel, grd, blk, 0, st, (const uint32_t* const*)d_round_ptrs, nr, idx->d_sa, n, idx->d_lcp);
  }
  mark("LCP from the ranks", st);
  TRY_HIP(dmalloc(&idx->d_klo, KTAB_ENTRIES));
  TRY_HIP(dmalloc(&idx->d_khi, KTAB_ENTRIES));
  TRY_HIP(hipMemsetAsync(idx->d_klo, 0, KTAB_ENTRIES * sizeof(uint32_t), st));
  TRY_HIP(hipMemsetAsync(idx->d_khi, 0, KTAB_ENTRIES * sizeof(uint32_t), st));
  if (n > 0) hipLaunchKernelGGL(kmer_table_kernel, grd, blk, 0, st, idx->d_gen, n, idx->d_sa, idx->d_klo, idx->d_khi);
  mark("8-mer table", st);
  TRY_HIP(build_lcf_tables(idx, genomic, st));
  TRY_HIP(hipStreamSynchronize(st));
  mark("packing + LCF tables", st);
  TRY_HIP(hipGetLastError());
done:
  hipFree(rank); hipFree(sa2); hipFree(flags); hipFree(newrank); hipFree(keys); hipFree(keys2); hipFree(tmp);
  for (uint32_t* q : round_ranks) hipFree(q);
  hipFree(d_round_ptrs);
  if (rc != PGPU_OK) { hipFree(idx->d_gen); hipFree(idx->d_sa); hipFree(idx->d_lcp); hipFree(idx->d_klo); hipFree(idx->d_khi); hipFree(idx->d_key); hipFree(idx->d_focc); hipFree(idx->d_rmq); hipFree(idx->d_code); hipFree(idx->d_bad); delete idx; return rc; }
  *out = idx;
  return PGPU_OK;
}

// ---- the index on disk: a gene is usually processed many times (parameter studies, re-runs of the
// pipeline), the index depends on the genomic sequence alone ------------------------------------
namespace {
// version 2: + checksum of the payload (a file whose header is right and whose tables are not -- torn by
// concurrent writers, truncated and padded, bit rot -- must not reach the device: an out-of-range
// suffix-array entry is an out-of-bounds read in every pairing kernel)
struct IndexFileHeader { char magic[8]; uint32_t version, ktab; uint64_t len, hash, payload_hash; };
const char INDEX_MAGIC[8] = { 'P', 'G', 'P', 'U', 'I', 'D', 'X', '1' };
constexpr uint32_t INDEX_VERSION = 2;
// word-wise FNV-style mix of the payload (1 Mb genomic = 9 MB of tables: a byte-wise loop would cost
// more than rebuilding the index)
uint64_t words_hash(const uint32_t* w, size_t n) {
  uint64_t h0 = 1469598103934665603ull, h1 = 0x9e3779b97f4a7c15ull;
  size_t i = 0;
  for (; i + 1 < n; i += 2) { h0 = (h0 ^ w[i]) * 1099511628211ull; h1 = (h1 ^ w[i + 1]) * 0x100000001b3ull; }
  if (i < n) h0 = (h0 ^ w[i]) * 1099511628211ull;
  return h0 ^ (h1 * 0xff51afd7ed558ccdull) ^ (uint64_t)n;
}
uint64_t fnv1a64(const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
}  // namespace

extern "C" int pgpu_index_save(pgpu_ctx* ctx, const pgpu_index* idx, const char* genomic, const char* path) {
  if (!ctx || !idx || !path || (idx->len && !genomic)) return PGPU_EINVAL;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  const size_t n = idx->len;
  std::vector<uint32_t> host(2 * n + 1 + 2 * (size_t)KTAB_ENTRIES);
  hipStream_t st = pgpu_ctx_stream(ctx);
  if ((n && hipMemcpyAsync(host.data(), idx->d_sa, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipMemcpyAsync(host.data() + n, idx->d_lcp, (n + 1) * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(host.data() + 2 * n + 1, idx->d_klo, KTAB_ENTRIES * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(host.data() + 2 * n + 1 + KTAB_ENTRIES, idx->d_khi, KTAB_ENTRIES * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return pgpu_ctx_fail(ctx, PGPU_EDEVICE, "index download failed");
  IndexFileHeader h;
  memcpy(h.magic, INDEX_MAGIC, 8); h.version = INDEX_VERSION; h.ktab = KTAB; h.len = n; h.hash = fnv1a64(genomic, n);
  h.payload_hash = words_hash(host.data(), host.size());
  // written under a temporary name of its OWN (several ranks, or several est-fact processes on the same
  // gene, may miss the cache and save at the same time) and renamed: a reader sees a whole file or none
  char tmpl[4200];
  if (snprintf(tmpl, sizeof tmpl, "%s.tmp.XXXXXX", path) >= (int)sizeof tmpl) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "index path too long");
  const int fd = mkstemp(tmpl);
  if (fd < 0) return pgpu_ctx_fail(ctx, PGPU_EINVAL, "cannot create the index file");
  (void)fchmod(fd, 0644);                      // mkstemp makes it 0600; a cache is shared like any other output file
  std::string tmp = tmpl;
  FILE* f = fdopen(fd, "wb");
  if (!f) { close(fd); remove(tmp.c_str()); return pgpu_ctx_fail(ctx, PGPU_EINVAL, "cannot create the index file"); }
  const bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(host.data(), 4, host.size(), f) == host.size();
  if (fclose(f) != 0 || !ok || rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); return pgpu_ctx_fail(ctx, PGPU_EDEVICE, "writing the index file failed"); }
  return PGPU_OK;
}

// PGPU_EINVAL when the file is missing, damaged or belongs to another sequence (the caller builds)
extern "C" int pgpu_index_load(pgpu_ctx* ctx, const char* path, const char* genomic, size_t len, pgpu_index** out) {
  if (!ctx || !path || !out || (len && !genomic)) return PGPU_EINVAL;
  *out = nullptr;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  FILE* f = fopen(path, "rb");
  if (!f) return PGPU_EINVAL;
  IndexFileHeader h;
  const size_t words = 2 * len + 1 + 2 * (size_t)KTAB_ENTRIES;
  std::vector<uint32_t> host;
  bool ok = fread(&h, sizeof h, 1, f) == 1 && memcmp(h.magic, INDEX_MAGIC, 8) == 0 && h.version == INDEX_VERSION && h.ktab == KTAB &&
            h.len == len && h.hash == fnv1a64(genomic, len);
  if (ok) { host.resize(words); ok = fread(host.data(), 4, words, f) == words && fgetc(f) == EOF; }
  fclose(f);
  if (ok) ok = h.payload_hash == words_hash(host.data(), words);
  // belt and braces: nothing that indexes the sequence or the suffix array may point outside
  for (size_t i = 0; ok && i < len; ++i) ok = host[i] < len;                                   // suffix array
  for (size_t i = 0; ok && i <= len; ++i) ok = host[len + i] <= len;                           // LCP
  for (size_t i = 0; ok && i < 2 * (size_t)KTAB_ENTRIES; ++i) ok = host[2 * len + 1 + i] <= len;   // k-mer intervals
  if (!ok) return PGPU_EINVAL;
  pgpu_index* idx = new (std::nothrow) pgpu_index();
  if (!idx) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of host memory");
  idx->len = len;
  hipStream_t st = pgpu_ctx_stream(ctx);
  const uint32_t n = (uint32_t)len;
  int rc = PGPU_OK;
  TRY_HIP(hipMalloc((void**)&idx->d_gen, len + 64));
  TRY_HIP(hipMemsetAsync(idx->d_gen, 0, len + 64, st));
  if (len) TRY_HIP(hipMemcpyAsync(idx->d_gen, genomic, len, hipMemcpyHostToDevice, st));
  TRY_HIP(upload_keys(idx, genomic, len, st));
  TRY_HIP(dmalloc(&idx->d_sa, n + 1)); TRY_HIP(dmalloc(&idx->d_lcp, n + 2));
  TRY_HIP(dmalloc(&idx->d_klo, KTAB_ENTRIES)); TRY_HIP(dmalloc(&idx->d_khi, KTAB_ENTRIES));
  if (n) TRY_HIP(hipMemcpyAsync(idx->d_sa, host.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(idx->d_lcp, host.data() + n, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(idx->d_klo, host.data() + 2 * (size_t)n + 1, KTAB_ENTRIES * 4, hipMemcpyHostToDevice, st));
  TRY_HIP(hipMemcpyAsync(idx->d_khi, host.data() + 2 * (size_t)n + 1 + KTAB_ENTRIES, KTAB_ENTRIES * 4, hipMemcpyHostToDevice, st));
  TRY_HIP(build_lcf_tables(idx, genomic, st));
  TRY_HIP(hipStreamSynchronize(st));
done:
  if (rc != PGPU_OK) { hipFree(idx->d_gen); hipFree(idx->d_sa); hipFree(idx->d_lcp); hipFree(idx->d_klo); hipFree(idx->d_khi); hipFree(idx->d_key); hipFree(idx->d_focc); hipFree(idx->d_rmq); hipFree(idx->d_code); hipFree(idx->d_bad); delete idx; return rc; }
  *out = idx;
  return PGPU_OK;
}

extern "C" int pgpu_index_destroy(pgpu_ctx* ctx, pgpu_index* idx) {
  if (!ctx || !idx) return PGPU_EINVAL;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStreamSynchronize(pgpu_ctx_stream(ctx));
  hipFree(idx->d_gen); hipFree(idx->d_sa); hipFree(idx->d_lcp); hipFree(idx->d_klo); hipFree(idx->d_khi); hipFree(idx->d_key);
  hipFree(idx->d_focc); hipFree(idx->d_rmq); hipFree(idx->d_code); hipFree(idx->d_bad);
  if (idx->lazy.tables && idx->lazy.release) idx->lazy.release(idx->lazy.tables);
  delete idx;
  return PGPU_OK;
}

extern "C" int pgpu_index_suffix_array(pgpu_ctx* ctx, const pgpu_index* idx, uint32_t* sa_out, size_t cap) {
  if (!ctx || !idx || !sa_out) return PGPU_EINVAL;
  if (cap < idx->len) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "suffix array buffer too small");
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  hipStream_t st = pgpu_ctx_stream(ctx);
  if (idx->len && (hipMemcpyAsync(sa_out, idx->d_sa, idx->len * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
                   hipStreamSynchronize(st) != hipSuccess))
    return pgpu_ctx_fail(ctx, PGPU_EDEVICE, "suffix array download failed");
  return PGPU_OK;
}
