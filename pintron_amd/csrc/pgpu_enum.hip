// Every candidate factorization of a MEG that need not be one path, from its record.  Semantics: include/pintron_gpu.h
// (pgpu_pairing_plan_run_candidate_lists, pgpu_index_candidate_lists): the root loop of get_EST_factorizations
// (src/est-factorizations.c:160-200), get_subtree_embeddings with its memo and its maximality pruning (:597-762, :1362-1460),
// update_embedding (:765-917) and the exons of get_factorizations_from_embeddings (:1292-1356).
//
//   enum_kernel<false>   one wave per record, one wave per workgroup, striding over the records: the enumeration, writing
//                        the result and the two counts (candidates, exons) for the scans.
//   enum_kernel<true>    behind two pgpu_exclusive_scan_u32: the enumeration again for the records of kind LISTS that have
//                        candidates, storing the candidate table and the exons into the compact arrays.
//
// The state of a record lives in LDS (struct State, 19 588 bytes per workgroup; tests/test_enum_resources.py):
//   pool   512 embeddings of 20 bytes.  An embedding is never copied: update_embedding fixes only the length of the node it adds
//          and the triple of the head it trims, and everything older is shared with the embedding it extends.  So an
//          embedding is the node's vertex and length, the trimmed head, the index of the embedding it extends and its
//          length; element 0 is the node, element i >= 1 the trimmed head of the ancestor i - 1 links up.  The copy the
//          source makes is an alias: the same index.  The pool only grows; 512 = PGPU_ENUM_MAX_EMBEDDINGS bounds it.
//   list   per vertex, at most 64 = PGPU_ENUM_MAX_LIST pool indices.
//   stack  the walk's own: at most 64 (vertex, next edge) pairs, since no vertex is on it twice.
//   vt, first   the record's vertices and CSR offsets; the targets are read where the record lies.
// Visited and on-stack are 64-bit masks in registers.  Everything the walk decides is the same in all lanes (held uniform
// with readfirstlane); lane 0 stores it and a barrier -- one wave, so it costs a wait -- stands between such a store and
// the loads of the other lanes.  The lanes are used where the work is wide: one lane per list entry computes
// maximality_relation(add, entry), and two ballots give k0 and the removal mask; one lane per cut runs the Burset scan, a
// maximum over (frequency, cut) keeping the last of equal cuts; one lane per candidate of a root counts and writes its exons.
// No atomics, nothing in HBM beside the call's blocks.  No scratch: the walk's counters and masks stay in registers (it enters a
// vertex at ONE place of the loop; entered through a lambda called from two, they lay in 128 bytes of scratch).
//
// Loop bounds, from nv <= 64, the record's edge count ne <= 65 535 (the CSR offsets are 16 bits wide) and the two caps:
//   roots                 nv
//   the walk per record   every turn enters a vertex (nv in all), leaves one (nv) or finishes an edge (ne): 2 nv + ne
//   folds per edge        the adjacent vertex's list: 64; so at most 64 ne folds per record, of which at most 512 return
//                         an embedding before the record is refused
//   the cut scan          ceil((hi - lo + 1) / 64) turns, hi - lo <= the shorter of the two pairings
//   maximality_relation   min(|add|, |cmp|) <= 64 steps along two chains of the pool
//   a candidate's exons   its embedding's length <= 64
#include <stdlib.h>
#include <string.h>

#include "pgpu_internal.h"
#include "pgpu_query_call.h"
#include "pgpu_stage_drive.h"
#include "pgpu_wave_dp.h"
#include "pgpu_burset.h"
#include "pgpu_enum.h"

namespace {

constexpr uint32_t MAX_V = PGPU_MEG_MAX_VERTICES, MAX_LIST = PGPU_ENUM_MAX_LIST, MAX_EMB = PGPU_ENUM_MAX_EMBEDDINGS;
static_assert(MAX_V == 64 && MAX_LIST == 64, "one bit per vertex, one lane per list entry");

struct Emb {
  int32_t node_l;              // the length update_embedding gave the node (element 0 = the vertex's p, t and this)
  int32_t th_p, th_t, th_l;    // the head it trimmed (element 1); unset when n == 1
  uint32_t link;               // parent | vertex << 16 | n << 24: the embedding it extends (unset when n == 1), the node's
                               // vertex, the embedding's length
  __device__ uint32_t parent() const { return link & 0xffffu; }
  __device__ uint32_t vertex() const { return link >> 16 & 0xffu; }
  __device__ uint32_t n() const { return link >> 24; }
};
__device__ inline uint32_t emb_link(uint32_t parent, uint32_t vertex, uint32_t n) { return parent | vertex << 16 | n << 24; }
struct State {
  Emb pool[MAX_EMB];
  uint16_t list[MAX_V][MAX_LIST];
  int32_t vt[3 * MAX_V];
  uint16_t first[MAX_V + 2];
  uint8_t len[MAX_V];
  uint8_t st_v[MAX_V];
  uint16_t st_e[MAX_V];
};
static_assert(sizeof(Emb) == 20 && sizeof(State) == 19588, "the LDS the head comment states");

__device__ inline uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ inline int unii(int x) { return __builtin_amdgcn_readfirstlane(x); }

struct Triple { int p, t, l; };
__device__ inline bool inside(const Triple& in, const Triple& out) {
  return !(in.p < out.p || in.p + in.l > out.p + out.l) && !(in.t < out.t || in.t + in.l > out.t + out.l);
}

// maximality_relation(add, cmp): 2 add is maximal, 1 both, 0 cmp is.  Per lane; at most 64 steps.
__device__ int relation(const State& S, uint32_t add, uint32_t cmp) {
  const uint32_t na = S.pool[add].n(), nc = S.pool[cmp].n(), m = na < nc ? na : nc;
  bool a_in_c = true, c_in_a = true;
  uint32_t a = add, c = cmp;
  Triple x = { S.vt[3 * S.pool[a].vertex()], S.vt[3 * S.pool[a].vertex() + 1], S.pool[a].node_l };
  Triple y = { S.vt[3 * S.pool[c].vertex()], S.vt[3 * S.pool[c].vertex() + 1], S.pool[c].node_l };
  for (uint32_t i = 0; i < m; ++i) {
    a_in_c = a_in_c && inside(x, y);
    c_in_a = c_in_a && inside(y, x);
    if ((!a_in_c && !c_in_a) || i + 1 == m) break;
    x.p = S.pool[a].th_p; x.t = S.pool[a].th_t; x.l = S.pool[a].th_l; a = S.pool[a].parent();
    y.p = S.pool[c].th_p; y.t = S.pool[c].th_t; y.l = S.pool[c].th_l; c = S.pool[c].parent();
  }
  if (na > nc) return c_in_a ? 2 : 1;
  if (na < nc) return a_in_c ? 0 : 1;
  return a_in_c ? 0 : (c_in_a ? 2 : 1);
}

// the exons of embedding x, front to back; WRITE: stored from `out` on.  Per lane; at most 64 steps.
template <bool WRITE>
__device__ uint32_t exons_of(const State& S, uint32_t x, int fl, pgpu_factor* out) {
  const uint32_t n = S.pool[x].n();
  uint32_t a = x, cnt = 0;
  int p = S.vt[3 * S.pool[a].vertex()], t = S.vt[3 * S.pool[a].vertex() + 1], l = S.pool[a].node_l;
  pgpu_factor f;
  f.EST_start = p; f.EST_end = p + l - 1; f.GEN_start = t; f.GEN_end = t + l - 1;
  for (uint32_t i = 1; i < n; ++i) {
    p = S.pool[a].th_p; t = S.pool[a].th_t; l = S.pool[a].th_l; a = S.pool[a].parent();
    if (t - f.GEN_end - 1 > fl) {
      if (WRITE) out[cnt] = f;
      ++cnt;
      f.EST_start = p; f.GEN_start = t;
    }
    f.EST_end = p + l - 1; f.GEN_end = t + l - 1;
  }
  if (WRITE) out[cnt] = f;
  return cnt + 1;
}

// the maximum of a 64-bit key over the wave, in all lanes
__device__ inline void wave_max_key(uint32_t& hi, uint32_t& lo) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t h2 = (uint32_t)__shfl_xor((int)hi, o), l2 = (uint32_t)__shfl_xor((int)lo, o);
    if (h2 > hi || (h2 == hi && l2 > lo)) { hi = h2; lo = l2; }
  }
}

// update_embedding(head-first embedding with this head, node): the fold step of pgpu_cand.hip with the cut scan one lane per
// cut.  All arguments and results are the same in every lane.
enum : int { F_NULL, F_ALIAS, F_SINGLE, F_EXTEND };
__device__ int fold_step(int head_p, int head_t, int head_l, int node_p, int node_t, int node_len, const uint8_t* __restrict__ T,
                         uint32_t tlen, int L, int min_intron, uint32_t lane, int& node_l, int& nh_p, int& nh_t, int& nh_l) {
  const int fl = 2 * L;
  node_l = node_len; nh_p = nh_t = nh_l = 0;
  if (head_p == CAND_SINK_P) return node_p < 0 ? F_NULL : F_SINGLE;
  if (node_p < 0) return F_ALIAS;                           // the source copies the embedding
  if (head_p < 0) return F_NULL;                            // a source as head: its deltas lie below 2L as integers (the header)
  const int small_delta = (head_p + head_l) - node_p;
  const int big_delta = (head_t + head_l) - node_t;
  if (!(small_delta >= fl && big_delta >= fl)) return F_NULL;
  if (!(small_delta - (node_len + head_l) <= fl)) return F_NULL;
  if (!((long long)small_delta - big_delta <= fl)) return F_NULL;
  if (small_delta >= node_len + head_l && big_delta >= node_len + head_l) {
    nh_p = head_p; nh_t = head_t; nh_l = head_l; node_l = node_len;
  } else {
    const int ref_delta = small_delta < big_delta ? small_delta : big_delta;
    int len_node = ref_delta / 2;
    int len_head = ref_delta - len_node;
    if (len_node > node_len) { len_node = node_len; len_head = ref_delta - len_node; }
    else if (len_head > head_l) { len_head = head_l; len_node = ref_delta - len_head; }
    nh_l = len_head;
    nh_p = head_p + head_l - nh_l;
    nh_t = head_t + head_l - nh_l;
    node_l = len_node;
  }
  const bool overlap_on_p = small_delta < node_len + head_l;
  const int gap_on_p = nh_p - node_p - node_l - 1;
  const int gap_on_t = nh_t - node_t - node_l - 1;
  const int intron_len = gap_on_t - (gap_on_p > 0 ? gap_on_p : 0);
  const bool intron_on_t = intron_len >= 0 && (min_intron == 0 || intron_len >= min_intron);
  if (overlap_on_p && intron_on_t) {
    // the best cut by Burset frequency, the last of equals: the maximum of (frequency + 1, cut); no cut leaves (0, 0)
    const int lo = node_p + L > head_p ? node_p + L : head_p;
    const int hi = head_p + head_l - L < node_p + node_len ? head_p + head_l - L : node_p + node_len;
    uint32_t kf = 0, kc = 0;
    for (int base = lo; base <= hi; base += 64) {          // (hi - lo) / 64 + 1 turns
      const int cut = base + (int)lane;
      if (cut <= hi && cut >= base) {                      // (cut >= base: base + lane did not wrap)
        const uint32_t f = 1u + (uint32_t)burset_adaptor(T, tlen, (uint32_t)(cut - node_p + node_t), (uint32_t)(cut - head_p + head_t));
        if (f > kf || (f == kf && (uint32_t)cut > kc)) { kf = f; kc = (uint32_t)cut; }
      }
      if (base > hi - 64) break;                           // the next base would pass hi (and must not wrap)
    }
    wave_max_key(kf, kc);
    const int best_cut = (int)kc;
    const int dH = best_cut - head_p;
    nh_l = head_l - dH; nh_p = head_p + dH; nh_t = head_t + dH;
    node_l = node_len - (node_p + node_len - best_cut);
  }
  if (!(gap_on_t <= fl || intron_on_t)) return F_NULL;
  return F_EXTEND;
}

template <bool WRITE>
__global__ __launch_bounds__(64)
void enum_kernel(const uint8_t* __restrict__ recs, const unsigned long long* __restrict__ rec_first, uint32_t n,
                 const uint8_t* __restrict__ T, uint32_t tlen, pgpu_cand_params prm, pgpu_enum_result* __restrict__ res,
                 uint32_t* __restrict__ cnt_c, uint32_t* __restrict__ cnt_e, const unsigned long long* __restrict__ first_c,
                 const unsigned long long* __restrict__ first_e, pgpu_enum_candidate* __restrict__ cands,
                 pgpu_factor* __restrict__ exons) {
  __shared__ State S;
  const uint32_t lane = threadIdx.x;
  const int L = (int)prm.min_factor_len, min_intron = prm.min_intron_length, fl = 2 * L;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint8_t* rec = recs + rec_first[i];
    const uint32_t* head = (const uint32_t*)rec;
    const uint32_t nv = uni(head[0]), flags = uni(head[2]);
    const bool flagged = (flags & (PGPU_MEG_UNAVAILABLE | PGPU_MEG_TOO_COMPLEX)) != 0 || nv > MAX_V;
    unsigned long long cbase = 0, ebase = 0;
    if (WRITE) {
      const uint4 r = *(const uint4*)&res[i];
      if ((r.x & 0xffffu) != PGPU_ENUM_LISTS || (r.w & 0xffffu) == 0) continue;
      cbase = first_c[i]; ebase = first_e[i];
      if (lane == 0) res[i].first_candidate = (uint32_t)cbase;
    } else if (flagged) {
      if (lane == 0) {
        *(uint4*)&res[i] = make_uint4(PGPU_ENUM_NONE, 0u, 0u, 0u);
        cnt_c[i] = 0; cnt_e[i] = 0;
      }
      continue;
    }
    const uint8_t* tgt = rec + 16 + 12 * (size_t)nv + 2 * ((size_t)nv + 1);
    __syncthreads();                                         // the record before this one has been read to its end
    if (lane < nv) {
      const int32_t* v3 = (const int32_t*)(rec + 16) + 3 * lane;
      S.vt[3 * lane] = v3[0]; S.vt[3 * lane + 1] = v3[1]; S.vt[3 * lane + 2] = v3[2];
      S.first[lane] = ((const uint16_t*)(rec + 16 + 12 * (size_t)nv))[lane];
    }
    if (lane == 0) S.first[nv] = ((const uint16_t*)(rec + 16 + 12 * (size_t)nv))[nv];
    __syncthreads();

    uint32_t kind = PGPU_ENUM_LISTS, detail = 0, work = 0, n_roots = 0, n_cands = 0, n_ex = 0, created = 0, pool_n = 0, sp = 0;
    unsigned long long visited = 0, onstack = 0;
    constexpr uint32_t NOBODY = MAX_V;
    for (uint32_t r = 0; r < nv && kind == PGPU_ENUM_LISTS; ++r) {       // nv roots at most
      if (visited >> r & 1ull) continue;
      ++n_roots;
      uint32_t to_enter = r;
      while (kind == PGPU_ENUM_LISTS) {                                  // 2 nv + ne turns at most
        if (to_enter != NOBODY) {
          // entering x: a vertex without out-edges has its one embedding at once and never lies on the stack
          const uint32_t x = to_enter;
          to_enter = NOBODY;
          visited |= 1ull << x;
          ++work;
          const uint32_t f0 = uni(S.first[x]), f1 = uni(S.first[x + 1]);
          if (f0 == f1) {
            if (++created > MAX_EMB) { kind = PGPU_ENUM_RANGE; detail = PGPU_ENUM_CAP_EMBEDDINGS; break; }
            if (lane == 0) {
              Emb& e = S.pool[pool_n];
              e.node_l = S.vt[3 * x + 2]; e.th_p = e.th_t = e.th_l = 0; e.link = emb_link(0xffffu, x, 1);
              S.list[x][0] = (uint16_t)pool_n; S.len[x] = 1;
            }
            ++pool_n;
          } else {
            onstack |= 1ull << x;
            if (lane == 0) { S.st_v[sp] = (uint8_t)x; S.st_e[sp] = (uint16_t)f0; S.len[x] = 0; }
            ++sp;
          }
          __syncthreads();
        }
        if (sp == 0) break;
        const uint32_t v = uni(S.st_v[sp - 1]), e = uni(S.st_e[sp - 1]);
        if (e == uni(S.first[v + 1])) { onstack &= ~(1ull << v); --sp; continue; }
        const uint32_t adj = uni(tgt[e]);
        if (!(visited >> adj & 1ull)) { to_enter = adj; continue; }
        if (onstack >> adj & 1ull) { kind = PGPU_ENUM_CYCLIC; break; }
        const uint32_t na = uni(S.len[adj]);
        uint32_t lv = uni(S.len[v]);
        const int node_p = unii(S.vt[3 * v]), node_t = unii(S.vt[3 * v + 1]), node_len = unii(S.vt[3 * v + 2]);
        for (uint32_t k = 0; k < na; ++k) {                              // 64 folds at most
          const uint32_t pe = uni(S.list[adj][k]);
          const uint32_t hv = uni(S.pool[pe].vertex());
          int node_l, nh_p, nh_t, nh_l;
          const int how = fold_step(unii(S.vt[3 * hv]), unii(S.vt[3 * hv + 1]), unii(S.pool[pe].node_l), node_p, node_t, node_len,
                                    T, tlen, L, min_intron, lane, node_l, nh_p, nh_t, nh_l);
          if (how == F_NULL) continue;
          ++work;
          if (++created > MAX_EMB) { kind = PGPU_ENUM_RANGE; detail = PGPU_ENUM_CAP_EMBEDDINGS; break; }
          uint32_t add = pe;
          if (how != F_ALIAS) {                                          // pool_n < created <= 512
            add = pool_n++;
            if (lane == 0) {
              Emb& x = S.pool[add];
              x.node_l = node_l; x.th_p = nh_p; x.th_t = nh_t; x.th_l = nh_l;
              x.link = how == F_EXTEND ? emb_link(pe, v, S.pool[pe].n() + 1) : emb_link(0xffffu, v, 1);
            }
            __syncthreads();
          }
          // the pruning: add against the list so far, one lane per entry
          const bool mine = lane < lv;
          const uint32_t entry = mine ? S.list[v][lane] : 0;
          const int rel = mine ? relation(S, add, entry) : 1;
          const unsigned long long zero = __ballot(mine && rel == 0), two = __ballot(mine && rel == 2);
          const unsigned long long gone = zero ? two & ((1ull << __builtin_ctzll(zero)) - 1ull) : two;
          if (gone) {
            __syncthreads();                                             // every lane has read its entry
            if (mine && !(gone >> lane & 1ull)) S.list[v][__builtin_popcountll(~gone & ((1ull << lane) - 1ull))] = (uint16_t)entry;
            lv -= (uint32_t)__builtin_popcountll(gone);
          }
          if (!zero) {
            if (lv == MAX_LIST) { kind = PGPU_ENUM_RANGE; detail = PGPU_ENUM_CAP_LIST; break; }
            if (lane == 0) S.list[v][lv] = (uint16_t)add;
            ++lv;
          }
          __syncthreads();
        }
        if (lane == 0) { S.len[v] = (uint8_t)lv; S.st_e[sp - 1] = (uint16_t)(e + 1); }
        __syncthreads();
      }
      if (kind != PGPU_ENUM_LISTS) break;
      // the root's candidates, one lane each
      const uint32_t lr = uni(S.len[r]);
      uint32_t x = 0, ne = 0;
      if (lane < lr) { x = S.list[r][lane]; ne = exons_of<false>(S, x, fl, nullptr); }
      uint32_t incl = ne;
      for (int o = 1; o < 64; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, o); if ((int)lane >= o) incl += y; }
      const uint32_t total = (uint32_t)__shfl((int)incl, 63);
      if (WRITE && lane < lr) {
        const unsigned long long at = ebase + n_ex + (incl - ne);
        // first_exon | n_exons, n_pairs | root | reserved
        *(uint4*)&cands[cbase + n_cands + lane] = make_uint4((uint32_t)at, ne | S.pool[x].n() << 16, r, 0u);
        exons_of<true>(S, x, fl, exons + at);
      }
      n_cands += lr; n_ex += total;
    }
    if (!WRITE && lane == 0) {
      // kind, detail | work | first_candidate | n_candidates, n_roots
      const bool ok = kind == PGPU_ENUM_LISTS;
      *(uint4*)&res[i] = make_uint4(kind | detail << 16, ok ? work : 0u, 0u, ok ? n_cands | n_roots << 16 : 0u);
      cnt_c[i] = ok ? n_cands : 0; cnt_e[i] = ok ? n_ex : 0;
    }
  }
}

thread_local double t_enum_ms = 0.0;

// the grid: sixteen waves per compute unit, never more than records
hipError_t enum_grid(uint32_t n, unsigned* blocks) {
  size_t waves = 0, cus = 0;
  const hipError_t e = chained_waves(n, waves, cus);
  *blocks = (unsigned)(waves ? waves : 1);
  return e;
}

}  // namespace

hipError_t pgpu_enum_launch_count(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                                  const pgpu_cand_params* prm, pgpu_enum_result* res, uint32_t* cnt_c, uint32_t* cnt_e, hipStream_t st) {
  if (n == 0) return hipSuccess;
  unsigned blocks = 1;
  DRIVE(enum_grid(n, &blocks));
  hipLaunchKernelGGL(enum_kernel<false>, dim3(blocks), dim3(64), 0, st, recs, rec_first, n, T, tlen, *prm, res, cnt_c, cnt_e,
                     (const unsigned long long*)nullptr, (const unsigned long long*)nullptr, (pgpu_enum_candidate*)nullptr,
                     (pgpu_factor*)nullptr);
  return hipSuccess;
}

hipError_t pgpu_enum_launch_write(const uint8_t* recs, const unsigned long long* rec_first, uint32_t n, const uint8_t* T, uint32_t tlen,
                                  const pgpu_cand_params* prm, pgpu_enum_result* res, const unsigned long long* first_c,
                                  const unsigned long long* first_e, pgpu_enum_candidate* cands, pgpu_factor* exons, hipStream_t st) {
  if (n == 0) return hipSuccess;
  unsigned blocks = 1;
  DRIVE(enum_grid(n, &blocks));
  hipLaunchKernelGGL(enum_kernel<true>, dim3(blocks), dim3(64), 0, st, recs, rec_first, n, T, tlen, *prm, res, (uint32_t*)nullptr,
                     (uint32_t*)nullptr, first_c, first_e, cands, exons);
  return hipSuccess;
}

extern "C" double pgpu_index_candidate_lists_kernel_ms(void) { return t_enum_ms; }

extern "C" int pgpu_index_candidate_lists(pgpu_ctx* ctx, const pgpu_index* idx, const void* records, size_t records_len,
                                          const uint64_t* rec_first, size_t n, const pgpu_cand_params* params,
                                          pgpu_enum_result* out, pgpu_enum_candidate* cands, size_t cands_cap,
                                          pgpu_factor* exons, size_t exons_cap, size_t* n_cands, size_t* n_exons) {
  t_enum_ms = 0.0;       // a refused call has no kernel time either
  static_assert(sizeof(pgpu_enum_result) == 16 && sizeof(pgpu_enum_candidate) == 16 && sizeof(pgpu_factor) == 16, "ABI layout");
  switch (enum_call_refusal(ctx, idx, records, records_len, rec_first, n, params, out, cands, cands_cap, exons, exons_cap, n_cands,
                            n_exons, idx ? pgpu_index_length(idx) : 0)) {
    case ENUM_OK: break;
    case ENUM_NULL: return PGPU_EINVAL;
    case ENUM_TOO_MANY: return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^31 - 1 records in one call");
    case ENUM_PARAMS: return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad candidate parameters (min_factor_len 0 or above 2^24)");
    default:
      return pgpu_ctx_fail(ctx, PGPU_EINVAL, "bad MEG record (offsets not ascending, past the buffer or not at a multiple of 4, a record "
                                             "shorter than its counts need, more than 64 vertices, CSR offsets out of order or past "
                                             "n_edges, a target that is no vertex, or a vertex outside what it indexes)");
  }
  *n_cands = 0; *n_exons = 0;
  if (n == 0) return PGPU_OK;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  QueryCall call(ctx, "candidate lists");
  const size_t rec_bytes = (size_t)rec_first[n];
  const EnumLayout E = enum_layout(rec_bytes, n, pgpu_scan_tmp_bytes(n + 1));
  TRY_HIP(hipMalloc((void**)&call.d, E.total));
  TRY_HIP(call.timing_events(2));
  if (rec_bytes) TRY_HIP(hipMemcpyAsync(call.d, records, rec_bytes, hipMemcpyHostToDevice, call.st));
  TRY_HIP(hipMemcpyAsync(call.d + E.first, rec_first, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, call.st));
  const uint8_t* const T = pgpu_index_genomic(idx);
  const uint32_t tlen = (uint32_t)pgpu_index_length(idx);
  pgpu_enum_result* const d_res = (pgpu_enum_result*)(call.d + E.res);
  uint32_t* const d_cnt_c = (uint32_t*)(call.d + E.cnt_c);
  uint32_t* const d_cnt_e = (uint32_t*)(call.d + E.cnt_e);
  unsigned long long* const d_off_c = (unsigned long long*)(call.d + E.off_c);
  unsigned long long* const d_off_e = (unsigned long long*)(call.d + E.off_e);
  const unsigned long long* const d_first = (const unsigned long long*)(call.d + E.first);
  TRY_HIP(call.record(0));
  TRY_HIP(pgpu_enum_launch_count(call.d, d_first, (uint32_t)n, T, tlen, params, d_res, d_cnt_c, d_cnt_e, call.st));
  TRY_HIP(drive_scan(d_cnt_c, d_off_c, n, call.d + E.tmp, call.st));
  TRY_HIP(drive_scan(d_cnt_e, d_off_e, n, call.d + E.tmp, call.st));
  TRY_HIP(call.record(1));
  unsigned long long total_c = 0, total_e = 0;
  TRY_HIP(hipMemcpyAsync(&total_c, d_off_c + n, sizeof total_c, hipMemcpyDeviceToHost, call.st));
  TRY_HIP(drive_total(ctx, d_off_e, n, &total_e));
  if (!enum_totals_fit(total_c, total_e))
    return pgpu_ctx_fail(ctx, PGPU_EINVAL, "more than 2^32 - 1 candidates or exons in one call");
  *n_cands = (size_t)total_c; *n_exons = (size_t)total_e;
  if (total_c > cands_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "candidate buffer too small");
  if (total_e > exons_cap) return pgpu_ctx_fail(ctx, PGPU_ENOSPC, "exon buffer too small");
  const EnumOutLayout O = enum_out_layout((size_t)total_c, (size_t)total_e);
  TRY_HIP(hipMalloc((void**)&call.d2, O.total));
  TRY_HIP(call.record(2));
  TRY_HIP(pgpu_enum_launch_write(call.d, d_first, (uint32_t)n, T, tlen, params, d_res, d_off_c, d_off_e,
                                 (pgpu_enum_candidate*)(call.d2 + O.cands), (pgpu_factor*)(call.d2 + O.exons), call.st));
  TRY_HIP(call.record(3));
  TRY_HIP(hipMemcpyAsync(out, d_res, n * sizeof(pgpu_enum_result), hipMemcpyDeviceToHost, call.st));
  if (total_c) TRY_HIP(hipMemcpyAsync(cands, call.d2 + O.cands, (size_t)total_c * sizeof(pgpu_enum_candidate), hipMemcpyDeviceToHost, call.st));
  if (total_e) TRY_HIP(hipMemcpyAsync(exons, call.d2 + O.exons, (size_t)total_e * sizeof(pgpu_factor), hipMemcpyDeviceToHost, call.st));
  TRY_HIP(pgpu_ctx_wait(ctx));
  TRY_HIP(hipGetLastError());
  double a = 0.0, b = 0.0;
  call.elapsed_ms(0, &a);
  call.elapsed_ms(1, &b);
  t_enum_ms = a + b;
  return PGPU_OK;
}
