// sample.hip -- on-device token sampling for the decode loop (reference
// /root/reference/models/stage2/generation.py:87-121 `sample`, the top_k > 0 branch and the top_k == 1 short cut).
//
// One 1024-thread workgroup per row of logits.  No host scalar is read after the launch, no allocation, no sync: the kernel
// sits inside the captured 1-token step (generation.SampleLoopGraph) and the per-step random stream comes from a device
// counter the graph itself advances.
//
//   top_k == 0      the whole vocabulary, multinomial of softmax(logits / T) (the reference's default arguments of t2i_generate:
//                   top_k = 0, top_p = 1.0).  Round 6: with the reference's two filters of this branch (generation.py:108-119) --
//                   min_p > 0: a token stays iff its raw logit >= min_p x the largest softmax(logits) probability (the reference compares
//                   LOGITS with that probability, :43; kept as it is) -- and 0 < top_p < 1: the ascending cumulative-probability cut of
//                   :57-69 over all V tokens WITHOUT a sort: token masses as 2^-40 fixed-point integers (sums do not depend on the order
//                   they are formed in), a 4-pass 8-bit radix walk over the order-preserving logit keys with MASS histograms finds the
//                   boundary value, ties at it are cut in index order, the draw is an inverse CDF over the kept tokens in index order.
//   top_k == 1      argmax (lowest index among equal maxima)
//   1 < top_k <= 64 the k largest logits by a 4-pass 8-bit radix select over order-preserving integer keys (histograms in LDS,
//                   the row re-read from L2: 200 KB of fp32 at vocab 50 288), candidates gathered into LDS and sorted by one
//                   wave (bitonic, ties by index); values / temperature; softmax over the k; top-p exactly as the reference
//                   filters -- a candidate stays iff the probability mass of the candidates LARGER than it is < top_p
//                   (generation.py:64-76: ascending cumulative sum <= 1 - top_p is cut; top_p <= 0 or >= 1 cuts nothing);
//                   inverse-CDF draw with one Philox4x32-10 uniform keyed by (seed, row, step counter).
// The reference draws with torch.multinomial; the streams differ, the distribution is the same (tests: chi-square at fixed
// seeds, bit-exact ids for top_k == 1).
#include <atomic>
#include "sample_select.h"

namespace omk {

struct SampleArgs {
  const void* logits; int64_t ls; int dt;
  int64_t* out; int B, V, top_k;
  float top_p, inv_temp, min_p;
  unsigned long long seed; const int64_t* counter; unsigned long long offset;
};

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1)
__device__ __forceinline__ void philox4x32(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t h0 = mulhi32(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
    const uint32_t h1 = mulhi32(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
constexpr int SAMPLE_KMAX = SELECT_NMAX;
// threads / waves per row of logits (round 6: 256 -> 1024, typed loads, four requests in flight per lane in every pass: the kernel is a chain
// of passes over one row from L2, bound by latency -- profiles/r06_sampler.txt).  The CPU emulator runs the same code with 256 (it executes the
// lanes one after the other: sixteen waves per row would make the CPU suite four times slower for nothing).
#ifdef OMK_EMU
constexpr int SNT = 256;
#else
constexpr int SNT = 1024;
#endif
constexpr int SNW = SNT / 64;

// inclusive scan over the SNT threads of the workgroup through LDS (buf: 2 x SNT entries); every thread returns its own prefix
template <class T>
__device__ __forceinline__ T block_incl_scan(T v, T* buf, int tid) {
  int cur = 0;
  buf[tid] = v;
  block_sync();
#pragma unroll 1
  for (int off = 1; off < SNT; off <<= 1) {
    T x = buf[cur * SNT + tid];
    if (tid >= off) x += buf[cur * SNT + tid - off];
    buf[(cur ^ 1) * SNT + tid] = x;
    cur ^= 1;
    block_sync();
  }
  const T r = buf[cur * SNT + tid];
  block_sync();
  return r;
}

// The settings of one row, uniform over its workgroup, in the two forms sample_row takes them in.  Both fill the four Philox counter
// words themselves: (first word, step low, step high, 0).
// omk_sample_rows: the row's entries of the device arrays.  c0 is the first counter word (0: the row index is not in the counter, see
// include/omk.h).
struct RowCfg {
  int top_k; float top_p, inv_temp, min_p;
  unsigned long long seed, step; uint32_t c0;
  float pen;   // SM_PEN / SM_EDIT only: what the logits marked in the id map are multiplied with (negative ones) / divided by
  int64_t* out;   // where the row's id goes
  __device__ __forceinline__ void philox_counter(uint32_t (&cc)[4]) const {
    cc[0] = c0; cc[1] = (uint32_t)step; cc[2] = (uint32_t)(step >> 32); cc[3] = 0u;
  }
  __device__ __forceinline__ void put(int64_t id) const { out[0] = id; }
};
// omk_sample: the kernel arguments of the whole batch and the row index, which is the first counter word.  The device counter is read
// HERE, at the draw, behind every pass over the row: the captured step advances it on the same stream in front of the launch.
struct BatchCfg {
  int top_k; float top_p, inv_temp, min_p;
  unsigned long long seed; const int64_t* counter; unsigned long long offset; int64_t* out; int row;
  static constexpr float pen = 1.f;
  __device__ __forceinline__ void philox_counter(uint32_t (&cc)[4]) const {
    const unsigned long long step = (counter ? (unsigned long long)counter[0] : 0ull) + offset;
    cc[0] = (uint32_t)row; cc[1] = (uint32_t)step; cc[2] = (uint32_t)(step >> 32); cc[3] = 0u;
  }
  // (indexed at every exit of the body.  Through a pointer made beforehand the compiler folds the exits into one store at the end of the
  // function, and that build measured +0.5 / +0.9 us a launch: profiles/sampler_one_body.txt section 3)
  __device__ __forceinline__ void put(int64_t id) const { out[row] = id; }
};

// What the row loader consults besides the row itself: nothing, the id map of the history, or the id map and the row's edit list.
constexpr int SM_NONE = 0, SM_PEN = 1, SM_EDIT = 2;
// Guided decoding: the row's token bitmask (one bit per token, LDS) behind whatever else the loader consults -- SM_MASK: nothing else (no id
// map: nothing to clear); SM_EDIT_MASK: SM_EDIT as it is with the bit array behind the list.  The id-map byte has no free bit left (below),
// so the mask has its own storage and its own instantiations.
constexpr int SM_MASK = 3, SM_EDIT_MASK = 4;
constexpr bool sm_edits(int mode) { return mode == SM_EDIT || mode == SM_EDIT_MASK; }
constexpr bool sm_masked(int mode) { return mode == SM_MASK || mode == SM_EDIT_MASK; }
// A byte of the id map.  Bit 0: the token is in the row's history.  SM_EDIT only -- bit 1: the token is in the row's edit list; bits 2 - 7:
// the BUCKET (entry index / EDIT_BUCKET) of the first entry that names it.  The loader reads the EDIT_BUCKET entries of that bucket and
// takes the first match: the first entry wins, in 8 LDS reads whatever the length of the list.  (Scanning the whole list instead, as first
// written, was a chain of dependent LDS reads per listed token and pass: +43 us a launch at 16 entries, 7 ms at 512 --
// profiles/sample_rows_edits.txt section 3.)
constexpr unsigned MAP_HIST = 1u, MAP_EDIT = 2u;
constexpr int EDIT_BUCKET = 8;
// SM_EDIT: the row's edit list as the preamble of sample_rows_kernel left it in LDS, whole buckets of it.  ids[j] is -1 where the entry's id
// is outside [0, V) and behind the row's length; allow: the row is allow-only and its list holds a valid id (uniform over the workgroup).
struct RowEdits { const int* ids; const float* vals; bool allow; };

#ifdef OMK_EMU
__device__ __forceinline__ uint32_t lds_cas_u32(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t o = *p; if (o == expect) *p = v; return o; }
#else
__device__ __forceinline__ uint32_t lds_cas_u32(uint32_t* p, uint32_t expect, uint32_t v) {
  __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return expect;
}
#endif
// Mark token `id` as listed by entry j: the byte keeps the lowest bucket among the entries that name the token (entries race for a byte, and
// a byte shares its word with three other tokens: a compare-and-swap on the word; every failure is another entry's success, so at most as
// many rounds as the list has entries).
__device__ __forceinline__ void map_mark_edit(unsigned char* map, int id, int j) {
  uint32_t* const w = (uint32_t*)map + (id >> 2);
  const int sh = 8 * (id & 3);
  const uint32_t mine = MAP_EDIT | ((uint32_t)(j / EDIT_BUCKET) << 2);
  uint32_t old = *w;
  for (;;) {
    const uint32_t ob = (old >> sh) & 0xffu;
    if ((ob & MAP_EDIT) && (ob >> 2) <= (mine >> 2)) return;
    const uint32_t now = (old & ~(0xffu << sh)) | (((ob & MAP_HIST) | mine) << sh);
    const uint32_t seen = lds_cas_u32(w, old, now);
    if (seen == old) return;
    old = seen;
  }
}

// One row of logits -> one id, by the whole workgroup: the one implementation behind omk_sample and omk_sample_rows.  MODE >= SM_PEN: `pmap`
// (LDS, one byte per token) marks the ids of the row's history; the loader penalises a marked logit and rounds it to T as the in-place torch
// version does, so every pass sees the same penalised row.  SM_EDIT: behind the penalty the loader adds the value of the first entry of `ed`
// that names the token (one more rounding to T), and an allow-only row reads -inf for every token its list does not name.  ALIASED picks the
// layout of the large LDS buffers, Cfg is RowCfg or BatchCfg.  SM_MASK / SM_EDIT_MASK: `bits` (LDS, ceil(V / 32) words) is the row's token
// mask, all ones for a row that ignores its mask; LAST in the loader, a token whose bit is clear reads -inf whatever the edits gave it.
template <class T, int MODE, bool ALIASED, class Cfg>
__device__ __forceinline__ void sample_row(const T* rowp, const int V, const Cfg a, const unsigned char* pmap, const RowEdits ed = {},
                                           const uint32_t* bits = nullptr) {
  // hist / hm8 / hc8: the counters of the radix passes, eight copies of every counter, picked by the lane: the keys of a row share their top
  // byte(s), and 64 lanes adding to ONE LDS address are 64 serial atomics (copy c of digit d lives at 8 d + c: the copies of a digit sit in
  // different banks).  sc64 / sc32 / scf: the buffers of the block scans.  Two layouts:
  //   ALIASED (omk_sample_rows, 44 792 B)  the branches are exclusive, so their buffers share two raw blocks:
  //              rawA  hist (top-k select)  |  hm8 + hc8 (whole-vocabulary top-p)
  //              rawB  sc64, sc32 (one after the other: a block scan ends with a barrier)  |  scf (plain whole-vocabulary draw)
  //            which leaves room for the id map of the penalty launch (50 288 B at the MMU vocabulary) next to them
  //   separate (omk_sample, 69 368 B)      an array each, as omk_sample always had.  It sits inside captured decode steps and has no id map
  //            to make room for, and this is the layout its per-launch time was measured with: not slower than the kernel it had to
  //            itself (profiles/sampler_one_body.txt section 3).  The aliased layout has not been measured for it on its own.
  // (a __shared__ array of the branch that is not taken is not allocated)
  uint32_t *hist, *hc8, *sc32;
  unsigned long long *hm8, *sc64;
  float* scf;
  if constexpr (ALIASED) {
    __shared__ __attribute__((aligned(16))) unsigned long long rawA[256 * 8 + 256 * 4];
    __shared__ __attribute__((aligned(16))) unsigned long long rawB[2 * SNT];
    hist = (uint32_t*)rawA; hm8 = rawA; hc8 = (uint32_t*)(rawA + 256 * 8);
    sc64 = rawB; sc32 = (uint32_t*)rawB; scf = (float*)rawB;
  } else {
    __shared__ uint32_t hist_s[256 * 8], hc8_s[256 * 8], sc32_s[2 * SNT];
    __shared__ unsigned long long hm8_s[256 * 8], sc64_s[2 * SNT];
    __shared__ float scf_s[2 * SNT];
    hist = hist_s; hm8 = hm8_s; hc8 = hc8_s; sc64 = sc64_s; sc32 = sc32_s; scf = scf_s;
  }
  __shared__ uint32_t sel_prefix, sel_need, n_gt, n_eq;
  __shared__ float cval[SAMPLE_KMAX];
  __shared__ int cidx[SAMPLE_KMAX];
  __shared__ float wmax[SNW];
  __shared__ int wimax[SNW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto ld = [&](int i) -> float {
    float v = to_f32(rowp[i]);
    if constexpr (MODE == SM_PEN) { if (pmap[i]) v = to_f32(from_f32<T>(v < 0.f ? v * a.pen : v / a.pen)); }
    if constexpr (sm_edits(MODE)) {
      const unsigned m = pmap[i];
      if (m & MAP_HIST) v = to_f32(from_f32<T>(v < 0.f ? v * a.pen : v / a.pen));
      if (m & MAP_EDIT) {
        // the first entry of the token's bucket that names it (there is one): from the back without an exit, so the reads do not wait for
        // the compares
        const int base = (int)(m >> 2) * EDIT_BUCKET;
        int jf = base;
#pragma unroll
        for (int u = EDIT_BUCKET - 1; u >= 0; u--) if (ed.ids[base + u] == i) jf = base + u;
        v = to_f32(from_f32<T>(v + ed.vals[jf]));
      } else if (ed.allow) v = -INFINITY;
    }
    // (in the strided passes 32 consecutive lanes read one word: a broadcast, not a bank conflict)
    if constexpr (sm_masked(MODE)) { if (!((bits[i >> 5] >> (i & 31)) & 1u)) v = -INFINITY; }
    return v;
  };
  // one pass over the row, thread-strided (coalesced), four requests in flight per lane
  auto strided = [&](auto&& fn) {
    for (int i0 = tid; i0 < V; i0 += 4 * SNT) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int i = i0 + u * SNT; v[u] = ld(i < V ? i : V - 1); }
#pragma unroll
      for (int u = 0; u < 4; u++) { const int i = i0 + u * SNT; if (i < V) fn(v[u], i); }
    }
  };
  // block maximum + its lowest index, in every thread
  auto block_argmax = [&](float& m, int& mi) {
    m = -INFINITY; mi = 0x7fffffff;
    strided([&](float v, int i) { if (v > m || (v == m && i < mi)) { m = v; mi = i; } });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float om = shfl_xor(m, off); const int oi = shfl_xor(mi, off);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (lane == 0) { wmax[wv] = m; wimax[wv] = mi; }
    block_sync();
    for (int k = 0; k < SNW; k++) if (wmax[k] > m || (wmax[k] == m && wimax[k] < mi)) { m = wmax[k]; mi = wimax[k]; }
  };
  auto philox_u24 = [&]() -> uint32_t {
    uint32_t cc[4];
    a.philox_counter(cc);
    philox4x32(cc, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    return cc[0] >> 8;
  };

  if (a.top_k == 1) {
    float m; int mi;
    block_argmax(m, mi);
    if (tid == 0) a.put(mi == 0x7fffffff ? 0 : mi);
    return;
  }
  if (a.top_k == 0 && (a.min_p > 0.f || (a.top_p > 0.f && a.top_p < 1.f))) {
    // ---- the whole vocabulary behind one of the reference's two filters (see the header)
    __shared__ unsigned long long hm[256];
    __shared__ uint32_t hc[256];
    __shared__ unsigned long long s_acc, s_ztot;
    __shared__ uint32_t s_prefix, s_r;
    __shared__ float wsumf[SNW];
    __shared__ int pick_f;
    const int c = (V + SNT - 1) / SNT, lo = tid * c < V ? tid * c : V, hi = lo + c < V ? lo + c : V;
    float m; int mi;
    if (tid == 0) pick_f = -1;
    block_argmax(m, mi);
    const float sct = a.inv_temp * LOG2E;
    // mass of a token in the tempered distribution, 2^-40 units of the largest one (an integer: sums are exact and order-free)
    auto mass = [&](float l) -> unsigned long long { return (unsigned long long)(exp2_fast((l - m) * sct) * 1099511627776.0f); };
    const bool use_min_p = a.min_p > 0.f;
    float thr = -INFINITY;           // min_p: raw logits below it are cut
    uint32_t vstar = 0u, rcut = 0u;  // top-p: keys below vstar are cut, and the first rcut tokens (index order) whose key equals it
    if (use_min_p) {
      float z = 0.f;
      strided([&](float v, int) { z += exp2_fast((v - m) * LOG2E); });          // softmax of the UNtempered logits (:109)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) z += shfl_xor(z, off);
      if (lane == 0) wsumf[wv] = z;
      block_sync();
      z = 0.f;
      for (int k = 0; k < SNW; k++) z += wsumf[k];
      thr = a.min_p / z;                                                        // max probability = 1 / z
    } else {
      unsigned long long zt = 0ull;
      strided([&](float v, int) { zt += mass(v); });
      const unsigned long long incl = block_incl_scan<unsigned long long>(zt, sc64, tid);
      if (tid == SNT - 1) s_ztot = incl;
      if (tid == 0) { s_prefix = 0u; s_acc = 0ull; }
      block_sync();
      const unsigned long long ztot = s_ztot;
      unsigned long long Q = (unsigned long long)((double)(1.f - a.top_p) * (double)ztot);   // masses <= Q (cumulative, ascending) are cut
      if (Q >= ztot) Q = ztot ? ztot - 1 : 0ull;
      for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 256 * 8; i += SNT) { hm8[i] = 0ull; hc8[i] = 0u; }
        block_sync();
        const uint32_t pre = s_prefix, pmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        strided([&](float l, int) {
          const uint32_t k = fkey(l);
          if ((k & pmask) == pre) { const uint32_t d = 8u * ((k >> shift) & 255u) + (uint32_t)(lane & 7); lds_add_u64(&hm8[d], mass(l)); lds_fetch_add_u32(&hc8[d], 1u); }
        });
        block_sync();
        if (tid < 256) {
          unsigned long long tm = 0ull; uint32_t tc = 0u;
#pragma unroll
          for (int c8 = 0; c8 < 8; c8++) { tm += hm8[8 * tid + c8]; tc += hc8[8 * tid + c8]; }
          hm[tid] = tm; hc[tid] = tc;
        }
        block_sync();
        if (wv == 0) {   // ascending: digits whose whole mass still fits under Q are cut; the first one that does not holds the boundary
          const unsigned long long acc0 = s_acc;
          uint32_t d; unsigned long long before;
          wave_find_digit<unsigned long long>([&](int rr) -> unsigned long long { return hm[rr]; }, Q - acc0, lane, d, before);
          if (lane == 0) {
            const unsigned long long acc = acc0 + before;
            s_acc = acc; s_prefix = pre | (d << shift);
            if (pass == 3) { const unsigned long long one = hc[d] ? hm[d] / hc[d] : 0ull; s_r = one ? (uint32_t)((Q - acc) / one) : 0u; if (s_r >= hc[d] && hc[d]) s_r = hc[d] - 1u; }
          }
        }
        block_sync();
      }
      vstar = s_prefix; rcut = s_r;
    }
    // ---- kept mass of the thread's tokens.  Ties at the boundary value that are cut (rare) need index-order ranks: contiguous slices then;
    // otherwise thread t owns t, t + SNT, ... (coalesced reads; the inverse CDF may lay the tokens out in any fixed order)
    const bool contig = !use_min_p && rcut > 0u;
    uint32_t tie_before = 0u;
    if (contig) {
      uint32_t tc = 0u;
      for (int i = lo; i < hi; i++) tc += fkey(ld(i)) == vstar ? 1u : 0u;
      tie_before = block_incl_scan<uint32_t>(tc, sc32, tid) - tc;
    }
    auto owned = [&](auto&& fn) {
      if (contig) { for (int i = lo; i < hi; i++) fn(ld(i), i); }
      else strided(fn);
    };
    unsigned long long km = 0ull;
    {
      uint32_t rank = tie_before;
      owned([&](float l, int) {
        bool keep;
        if (use_min_p) keep = l >= thr;
        else { const uint32_t k = fkey(l); keep = k > vstar || (k == vstar && rank++ >= rcut); }
        if (keep) km += mass(l);
      });
    }
    const unsigned long long incl = block_incl_scan<unsigned long long>(km, sc64, tid);
    if (tid == SNT - 1) s_ztot = incl;
    block_sync();
    const unsigned long long ktot = s_ztot, start = incl - km;
    const unsigned long long u24 = philox_u24();
    const unsigned long long target = (ktot >> 24) * u24 + (((ktot & 0xffffffull) * u24) >> 24);   // floor(u ktot), u in [0, 1): < ktot
    if (ktot > 0ull && target >= start && target < incl) {   // exactly one thread
      unsigned long long run = start; uint32_t rank = tie_before; int got = -1; bool done = false;
      owned([&](float l, int i) {
        bool keep;
        if (use_min_p) keep = l >= thr;
        else { const uint32_t k = fkey(l); keep = k > vstar || (k == vstar && rank++ >= rcut); }
        const unsigned long long e = keep ? mass(l) : 0ull;
        if (!done && e > 0ull) got = i;
        run += e;
        if (run > target) done = true;
      });
      pick_f = got;
    }
    block_sync();
    // (nothing kept -- min_p with every logit under the threshold, where the reference's multinomial raises on a row of NaN: the arg max)
    if (tid == 0) a.put(pick_f >= 0 ? pick_f : (mi == 0x7fffffff ? 0 : mi));
    return;
  }
  if (a.top_k == 0) {
    // full-vocabulary multinomial (the reference's top_k == 0 branch with top_p outside (0, 1): softmax(logits / T), one draw).
    // Block maximum, the mass of every thread's tokens, an inclusive scan of the SNT masses (the scan values tile [0, total) exactly:
    // end_t = start_{t + 1}), one Philox number scaled to the total, and the thread whose interval holds it walks its tokens.
    __shared__ float tot_s;
    __shared__ int pick_s;
    // (thread t owns the tokens t, t + SNT, ...: the inverse CDF may lay the tokens out in ANY fixed order, and this one reads coalesced --
    // contiguous slices per thread were 64 scattered lines per request: 17 -> see profiles/r06_sampler.txt)
    float m; int mi;
    if (tid == 0) pick_s = 0;
    block_argmax(m, mi);
    const float sc = a.inv_temp * LOG2E;
    float mine = 0.f;
    strided([&](float v, int) { mine += exp2_fast((v - m) * sc); });
    const float end = block_incl_scan<float>(mine, scf, tid);
    scf[tid] = end;                                                 // (the scan values tile [0, total): a thread starts where its neighbour ends)
    if (tid == SNT - 1) tot_s = end;
    block_sync();
    const float tot = tot_s, start = tid ? scf[tid - 1] : 0.f;
    float u = (float)philox_u24() * (1.0f / 16777216.0f) * tot;   // uniform in [0, tot)
    if (u >= tot) u = tot * 0.99999994f;                            // (the product may round up to the total)
    if (u >= start && u < end) {   // exactly one thread when 0 < tot < inf
      float run = start; int got = tid < V ? tid : 0; bool done = false;
      strided([&](float v, int i) {
        const float e = exp2_fast((v - m) * sc);
        if (!done && e > 0.f) got = i;                              // rounding inside the walk: the last token with mass
        run += e;
        if (run > u) done = true;
      });
      pick_s = got;
    }
    block_sync();
    if (tid == 0) a.put(pick_s);
    return;
  }
  const int K = a.top_k < V ? a.top_k : V;
  // ---- radix select: the key of the K-th largest logit, 8 bits per pass from the top
  // (this loop, the walk over the ties and the sort below are repeated in token_logprobs.hip: as templates of sample_select.h each changed the
  // instruction sequences of both files' kernels)
  if (tid == 0) { sel_prefix = 0u; sel_need = (uint32_t)K; }
  for (int pass = 0; pass < 4; pass++) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 256 * 8; i += SNT) hist[i] = 0u;
    block_sync();
    const uint32_t pre = sel_prefix, pmask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
    strided([&](float v, int) {   // (aggregating the lanes of a wave per distinct digit with ballots instead: slower, 55.7 -> 66.3 us)
      const uint32_t k = fkey(v);
      if ((k & pmask) == pre) lds_fetch_add_u32(&hist[8u * ((k >> shift) & 255u) + (uint32_t)(lane & 7)], 1u);
    });
    block_sync();
    if (tid < 256) {
      uint32_t t = 0u;
#pragma unroll
      for (int c = 0; c < 8; c++) t += hist[8 * tid + c];
      hist[8 * tid] = t;
    }
    block_sync();
    if (wv == 0) {   // walk the digits from the top until `need` keys are covered
      const uint32_t need = sel_need;
      uint32_t r, before;
      wave_find_digit<uint32_t>([&](int rr) -> uint32_t { return hist[8u * (255u - (uint32_t)rr)]; }, need - 1u, lane, r, before);
      if (lane == 0) { sel_prefix = pre | ((255u - r) << shift); sel_need = need - before; }
    }
    block_sync();
  }
  const uint32_t kth = sel_prefix;           // keys > kth: all taken; keys == kth: sel_need of them (lowest indices first)
  const uint32_t take_eq = sel_need;
  if (tid == 0) { n_gt = 0u; n_eq = 0u; }
  block_sync();
  const uint32_t base_eq = (uint32_t)K - take_eq;   // slots [0, base_eq) for keys > kth, [base_eq, K) for the ties at the threshold
  strided([&](float v, int i) {
    const uint32_t k = fkey(v);
    if (k > kth) { const uint32_t s = lds_fetch_add_u32(&n_gt, 1u); if (s < base_eq) { cval[s] = v; cidx[s] = i; } }
    else if (k == kth) { const uint32_t s = lds_fetch_add_u32(&n_eq, 1u); if (s < take_eq) { cval[base_eq + s] = v; cidx[base_eq + s] = i; } }
  });
  block_sync();
  if (wv != 0) return;
  if (n_eq > take_eq) {
    // more logits equal the threshold than there are slots left (16-bit logits tie often): which of them are candidates must not
    // depend on the order the tickets were handed out -- one wave walks the row in index order and keeps the first take_eq
    uint32_t got = 0u;
    for (int i0 = 0; i0 < V && got < take_eq; i0 += 64) {
      const int i = i0 + lane;
      float v = 0.f;
      bool eq = false;
      if (i < V) { v = ld(i); eq = fkey(v) == kth; }
      const unsigned long long m = ballot64(eq);
      const uint32_t rank = got + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (eq && rank < take_eq) { cval[base_eq + rank] = v; cidx[base_eq + rank] = i; }
      got += (uint32_t)__builtin_popcountll(m);
    }
  }
  // ---- one wave: sort the K candidates (value descending, index ascending), softmax, top-p, draw
  float v = lane < K ? cval[lane] : -INFINITY;
  int ix = lane < K ? cidx[lane] : 0x7fffffff;
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      const float ov = shfl_xor(v, stride); const int oi = shfl_xor(ix, stride);
      const bool first = (lane & stride) == 0;                  // lower lane of the pair
      const bool desc = (lane & size) == 0;                     // direction of this bitonic block
      const bool mine_before = v > ov || (v == ov && ix < oi);  // "mine sorts before the other" in descending order
      const bool keep = (first == desc) ? mine_before : !mine_before;
      if (!keep) { v = ov; ix = oi; }
    }
  const float vmax = wave_read_lane(v, 0);
  float p = lane < K ? exp2_fast((v - vmax) * a.inv_temp * LOG2E) : 0.f;
  const float tot = wave_sum(p);
  p /= tot;
  float incl = wave_incl_scan_add(p);
  const float excl = incl - p;
  const bool keep = lane < K && (a.top_p <= 0.f || a.top_p >= 1.f || excl < a.top_p);
  const float pk = keep ? p : 0.f;
  const float ktot = wave_sum(pk);
  const float cum = wave_incl_scan_add(pk);
  const float u = (float)philox_u24() * (1.0f / 16777216.0f) * ktot;   // uniform in [0, ktot)
  // first kept candidate whose cumulative mass exceeds u
  const bool hit = keep && cum > u;
  const unsigned long long mask = ballot64(hit);
  int pick = mask ? __builtin_ctzll(mask) : 0;   // rounding at the top end: fall back to the largest candidate
  const int chosen = shfl(ix, pick);
  if (lane == 0) a.put(chosen);
}

// omk_sample: the whole-batch settings are kernel arguments (one round of scalar loads), and the row index goes into the Philox counter.
// sample_row's body with the separate LDS arrays.  The kernel sits inside captured steps: its registers and LDS are those it had as a body
// of its own (56 VGPRs, 66 SGPRs, 69 368 B, no scratch), its per-launch time is not above that body's (profiles/sampler_one_body.txt).
template <class T>
__global__ __launch_bounds__(SNT) void sample_kernel(SampleArgs a) {
  const int row = blockIdx.x;
  const BatchCfg c = {a.top_k, a.top_p, a.inv_temp, a.min_p, a.seed, a.counter, a.offset, a.out, row};
  sample_row<T, SM_NONE, false>((const T*)a.logits + (int64_t)row * a.ls, a.V, c, nullptr);
}

// SM_EDIT: bytes of the id map (the edit list behind it starts on a 16-byte boundary) and entries of the list's LDS copy (whole buckets)
__host__ __device__ constexpr size_t edit_map_bytes(int V) { return (size_t)((V + 15) / 16) * 16; }
__host__ __device__ constexpr int edit_lds_entries(int ecap) { return (ecap + EDIT_BUCKET - 1) / EDIT_BUCKET * EDIT_BUCKET; }

struct SampleRowsArgs {
  const void* logits; int64_t ls;
  int64_t* out; int V;
  const int* top_k; const float *top_p, *temperature, *min_p;
  const unsigned long long* seeds; const int64_t* steps;
  const float* penalty; const int64_t* history; const int* history_lens; const int* active;
  int64_t hs; int hcap;
  const int64_t* edit_ids; const float* edit_vals; const int* edit_lens; const int* edit_mode;   // SM_EDIT only
  int64_t es; int ecap;
  const uint32_t* mask; const int* mask_on; int64_t ms;   // SM_MASK / SM_EDIT_MASK only (behind everything the older instantiations read)
};

// words of a row's token mask in LDS
__host__ __device__ constexpr int mask_lds_words(int V) { return (V + 31) / 32; }

// omk_sample_rows: row b's settings come from the device arrays.  Nothing in them is trusted: see the clamps (include/omk.h).
// MODE >= SM_PEN: dynamic LDS holds the id map of the row's history, (V rounded up to 4) bytes.  SM_EDIT: the map (V rounded up to 16 bytes),
// behind it the row's edit list in whole buckets (edit_lds_entries(ecap) ids as int32, as many values) and one word that says whether any of
// its ids was valid.  SM_MASK: dynamic LDS holds the row's mask_lds_words(V) mask words and nothing else.  SM_EDIT_MASK: the SM_EDIT layout
// with the mask words behind the any-valid word; a.ecap == 0 is legal (a history with a mask and no list: no bucket, allow false).
template <class T, int MODE>
__global__ __launch_bounds__(SNT) void sample_rows_kernel(SampleRowsArgs a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  // The row's entries are all requested in ONE round of scalar loads, the active flag among them: nothing of the passes over the row
  // can start before the branch is known, so a flag tested first puts its own rounds (its pointer, then its value) in front of the
  // round of the settings.  The compiler sinks the loads behind the test when it may: the OMK_OPAQUE_S lines pin them in front of it.
  // An inactive row's entries are inside the (batch) arrays like every row's; what they hold is not looked at.
  int act = *(a.active ? a.active + row : a.top_k + row);   // (no flag array: any valid word, so the load needs no branch of its own)
  int k = a.top_k[row];
  float tp = a.top_p[row], t = a.temperature[row], mp = a.min_p[row];
  unsigned long long sd = a.seeds[row], st = (unsigned long long)a.steps[row];
  int mon = 1;   // SM_MASK / SM_EDIT_MASK: the row's mask_on entry joins the same round (no array: every row is masked)
  if constexpr (sm_masked(MODE)) mon = *(a.mask_on ? a.mask_on + row : a.top_k + row);
  OMK_OPAQUE_S(k); OMK_OPAQUE_S(tp); OMK_OPAQUE_S(t); OMK_OPAQUE_S(mp); OMK_OPAQUE_S(sd); OMK_OPAQUE_S(st); OMK_OPAQUE_S(act);
  if constexpr (sm_masked(MODE)) OMK_OPAQUE_S(mon);
  if (a.active && act == 0) return;   // (uniform over the workgroup, in front of every barrier)
  RowCfg c;
  c.top_k = uniform_i(k < 0 ? 0 : (k > SAMPLE_KMAX ? SAMPLE_KMAX : k));   // (the clamp is a VALU v_med3: back into a scalar register, as omk_sample's argument is)
  c.top_p = tp;
  c.inv_temp = t > 0.f ? 1.f / t : 1.f;
  c.min_p = c.top_k == 0 ? mp : 0.f;
  c.seed = sd; c.step = st; c.c0 = 0u; c.pen = 1.f; c.out = a.out + row;
  const unsigned char* pmap = nullptr;
  RowEdits ed = {};
  const uint32_t* bits = nullptr;
  // The row's mask words into LDS, all ones for a row that ignores its mask (mask_on[row] == 0): the loader stays uniform, no "is this row
  // masked" test in the passes.  An unmasked row does not read its mask row.  (The caller's barrier publishes the words.)
  auto stage_mask = [&](uint32_t* w) {
    const bool masked = !a.mask_on || mon != 0;
    const uint32_t* mrow = a.mask + (int64_t)row * a.ms;
    for (int i = tid; i < mask_lds_words(a.V); i += SNT) w[i] = masked ? mrow[i] : 0xffffffffu;
  };
  if constexpr (MODE == SM_MASK) {
    OMK_DYN_SMEM(dyn);
    stage_mask((uint32_t*)dyn);
    block_sync();
    bits = (const uint32_t*)dyn;
  }
  if constexpr (MODE == SM_PEN) {
    OMK_DYN_SMEM(dyn);
    unsigned char* const map = (unsigned char*)dyn;
    const float pen = a.penalty[row];
    int hl = a.history_lens[row];
    hl = hl < 0 ? 0 : (hl > a.hcap ? a.hcap : hl);
    if (!(pen > 0.f) || pen == 1.f) hl = 0;     // off: an empty map
    else c.pen = pen;
    for (int i = tid; i < (a.V + 3) / 4; i += SNT) ((uint32_t*)map)[i] = 0u;
    block_sync();
    const int64_t* hrow = a.history + (int64_t)row * a.hs;
    for (int j = tid; j < hl; j += SNT) { const int64_t id = hrow[j]; if (id >= 0 && id < (int64_t)a.V) map[id] = 1; }   // plain stores of 1: duplicates mark once
    block_sync();
    pmap = map;
  }
  if constexpr (sm_edits(MODE)) {
    OMK_DYN_SMEM(dyn);
    unsigned char* const map = (unsigned char*)dyn;
    const int ecap8 = edit_lds_entries(a.ecap);
    int* const eids = (int*)(dyn + edit_map_bytes(a.V));
    float* const evals = (float*)(eids + ecap8);
    uint32_t* const any_valid = (uint32_t*)(evals + ecap8);
    // (the penalty and the history are optional here: a launch with edits alone marks no history)
    const float pen = a.penalty ? a.penalty[row] : 1.f;
    int hl = a.history ? a.history_lens[row] : 0;
    int el;
    if constexpr (MODE == SM_EDIT_MASK) el = a.ecap > 0 ? a.edit_lens[row] : 0;   // (a mask and a history without a list)
    else el = a.edit_lens[row];
    const int em = a.edit_mode ? a.edit_mode[row] : 0;
    hl = hl < 0 ? 0 : (hl > a.hcap ? a.hcap : hl);
    el = el < 0 ? 0 : (el > a.ecap ? a.ecap : el);
    if (!(pen > 0.f) || pen == 1.f) hl = 0;     // off: no history mark
    else c.pen = pen;
    for (int i = tid; i < (a.V + 3) / 4; i += SNT) ((uint32_t*)map)[i] = 0u;
    if (tid == 0) *any_valid = 0u;
    if constexpr (MODE == SM_EDIT_MASK) { stage_mask(any_valid + 1); bits = any_valid + 1; }
    block_sync();
    const int64_t* hrow = a.history + (int64_t)row * a.hs;
    for (int j = tid; j < hl; j += SNT) { const int64_t id = hrow[j]; if (id >= 0 && id < (int64_t)a.V) map[id] = (unsigned char)MAP_HIST; }
    block_sync();   // (the history marks are whole-byte stores: they are done before the words of the map are swapped)
    const int64_t* irow = a.edit_ids + (int64_t)row * a.es;
    const float* vrow = a.edit_vals + (int64_t)row * a.es;
    for (int j = tid; j < ecap8; j += SNT) {   // (whole buckets: the entries behind the row's length read as "no token")
      const int64_t id = j < el ? irow[j] : -1;
      const bool ok = id >= 0 && id < (int64_t)a.V;
      eids[j] = ok ? (int)id : -1;
      evals[j] = j < el ? vrow[j] : 0.f;
      if (ok) { map_mark_edit(map, (int)id, j); *any_valid = 1u; }
    }
    block_sync();
    ed.ids = eids; ed.vals = evals;
    ed.allow = em == 1 && uniform_i((int)*any_valid) != 0;   // allow-only without a valid id: unconstrained
    pmap = map;
  }
  sample_row<T, MODE, true>((const T*)a.logits + (int64_t)row * a.ls, a.V, c, pmap, ed, bits);
}

}  // namespace omk

using namespace omk;

extern "C" int omk_sample(const OmkSample* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->logits) && present(p->out_ids), "sample: logits and out_ids required");
  OMK_REQUIRE(p->logits.ndim == 2 && p->logits.stride[1] == 1, "sample: logits must be (batch, vocab) with unit last stride");
  OMK_REQUIRE(p->out_ids.ndim == 1 && p->out_ids.shape[0] == p->logits.shape[0] && p->out_ids.stride[0] == 1, "sample: out_ids must be dense int64 (batch)");
  OMK_REQUIRE(p->logits.dtype == OMK_F32 || p->logits.dtype == OMK_BF16 || p->logits.dtype == OMK_F16, "sample: logits dtype");
  OMK_REQUIRE(p->top_k >= 0 && p->top_k <= SAMPLE_KMAX, "sample: top_k must be in [0, %d]", SAMPLE_KMAX);
  OMK_REQUIRE(p->min_p >= 0.f && p->min_p < 1.f, "sample: min_p must be in [0, 1)");
  OMK_REQUIRE(p->min_p == 0.f || p->top_k == 0, "sample: min_p belongs to the whole-vocabulary branch (top_k == 0), as in the reference");
  OMK_REQUIRE(p->temperature > 0.f, "sample: temperature must be positive");
  OMK_REQUIRE(p->top_p <= 1.f, "sample: top-p should be in (0, 1]");
  if (p->logits.shape[0] == 0) return OMK_OK;
  OMK_REQUIRE(p->logits.shape[1] > 0 && p->logits.shape[1] < (1ll << 31), "sample: vocabulary size");
  SampleArgs a = {};
  a.logits = p->logits.data; a.ls = p->logits.stride[0]; a.dt = p->logits.dtype;
  a.out = (int64_t*)p->out_ids.data; a.B = (int)p->logits.shape[0]; a.V = (int)p->logits.shape[1]; a.top_k = p->top_k;
  a.top_p = p->top_p; a.inv_temp = 1.f / p->temperature; a.min_p = p->min_p;
  a.seed = p->seed; a.counter = (const int64_t*)p->step_counter; a.offset = p->offset;
  dim3 grid((unsigned)a.B), block(SNT);
  OMK_DISPATCH_DTYPE(a.dt, T, OMK_LAUNCH((sample_kernel<T>), grid, block, 0, stream, a));
  return finish_launch("sample");
}

// the id map of the penalty launch: one byte per token in dynamic LDS, next to the 44 KB the branches share
constexpr int64_t SAMPLE_PEN_MAX_V = 65536;

// the edit list of the SM_EDIT launch: 8 bytes per entry in dynamic LDS behind the id map.  44 800 B static + 65 536 B of map + 8 x 512 B + one
// word = 114 436 B of the 163 840 B a workgroup may hold.  64 buckets: what the six bits of a map byte name.
constexpr int64_t SAMPLE_EDIT_MAX = 64 * EDIT_BUCKET;

// Raise the dynamic-LDS limit of an instantiation with an id map when a launch needs more than the device was already granted, not on
// every step (the attribute belongs to a function on a device).  0 = granted.
template <class T, int MODE> static int grant_map_lds(size_t smem) {
#ifdef OMK_EMU
  return 0;
#else
  constexpr int MAXDEV = 64;
  static std::atomic<size_t> granted[MAXDEV];
  int d = -1;
  const bool known = hipGetDevice(&d) == hipSuccess && d >= 0 && d < MAXDEV;
  if (known && granted[d].load(std::memory_order_relaxed) >= smem) return 0;
  if (OMK_SET_MAX_DYN_SMEM((sample_rows_kernel<T, MODE>), smem)) return 1;
  if (known) granted[d].store(smem, std::memory_order_relaxed);
  return 0;
#endif
}

// THE selector of omk_sample_rows: every check of a call, the kernel arguments and which instantiation takes it -- omk_sample_rows launches
// what this says, omk_sample_rows_form reports it.  Returns OMK_SAMPLE_ROWS_* or the negative omk_status of a call that is refused.
namespace {
struct SampleRowsPlan {
  SampleRowsArgs a;
  bool empty;      // no row: nothing to launch
  size_t smem;     // dynamic LDS
};
}  // namespace

static int sample_rows_plan(const OmkSampleRows* p, SampleRowsPlan& pl) {
  OMK_REQUIRE(p && present(p->logits) && present(p->out_ids), "sample_rows: logits and out_ids required");
  OMK_REQUIRE(p->logits.ndim == 2 && p->logits.stride[1] == 1, "sample_rows: logits must be (batch, vocab) with unit last stride");
  OMK_REQUIRE(p->out_ids.ndim == 1 && p->out_ids.shape[0] == p->logits.shape[0] && p->out_ids.stride[0] == 1, "sample_rows: out_ids must be dense int64 (batch)");
  OMK_REQUIRE(p->logits.dtype == OMK_F32 || p->logits.dtype == OMK_BF16 || p->logits.dtype == OMK_F16, "sample_rows: logits dtype");
  OMK_REQUIRE(p->top_k && p->top_p && p->temperature && p->min_p && p->seeds && p->steps,
              "sample_rows: top_k, top_p, temperature, min_p, seeds and steps are required device arrays of (batch) entries");
  OMK_REQUIRE(!p->history || p->history_lens, "sample_rows: history needs history_lens");
  OMK_REQUIRE(!p->history || (p->history_cap >= 0 && p->history_cap < (1ll << 31)), "sample_rows: history_cap");
  OMK_REQUIRE(!p->edit_ids || (p->edit_vals && p->edit_lens), "sample_rows: edit_ids needs edit_vals and edit_lens");
  OMK_REQUIRE(!p->edit_ids || (p->edit_cap >= 0 && p->edit_cap < (1ll << 31)), "sample_rows: edit_cap");
  pl = SampleRowsPlan{};
  SampleRowsArgs& a = pl.a;
  const bool pen = p->penalty && p->history && p->history_cap > 0;   // (no penalty array, or no history: nothing to penalise)
  const bool edit = p->edit_ids && p->edit_cap > 0;                  // (no edit array, or no room in it: today's launch)
  const int form = edit ? OMK_SAMPLE_ROWS_EDIT : (pen ? OMK_SAMPLE_ROWS_PENALTY : OMK_SAMPLE_ROWS_PLAIN);
  if (p->logits.shape[0] == 0) { pl.empty = true; return form; }
  OMK_REQUIRE(p->logits.shape[1] > 0 && p->logits.shape[1] < (1ll << 31), "sample_rows: vocabulary size");
  a.logits = p->logits.data; a.ls = p->logits.stride[0];
  a.out = (int64_t*)p->out_ids.data; a.V = (int)p->logits.shape[1];
  a.top_k = (const int*)p->top_k; a.top_p = (const float*)p->top_p; a.temperature = (const float*)p->temperature; a.min_p = (const float*)p->min_p;
  a.seeds = (const unsigned long long*)p->seeds; a.steps = (const int64_t*)p->steps; a.active = (const int*)p->active;
  if (form == OMK_SAMPLE_ROWS_PLAIN) return form;
  if (a.V > SAMPLE_PEN_MAX_V)
    return fail(OMK_EUNSUPPORTED, "sample_rows: the id map of the repetition penalty and the edits holds %lld tokens, the vocabulary has %d", (long long)SAMPLE_PEN_MAX_V, a.V);
  if (pen) {
    a.penalty = (const float*)p->penalty; a.history = (const int64_t*)p->history; a.history_lens = (const int*)p->history_lens;
    a.hs = p->history_stride; a.hcap = (int)p->history_cap;
  }
  pl.smem = (size_t)((a.V + 3) / 4) * 4;
  if (!edit) return form;
  if (p->edit_cap > SAMPLE_EDIT_MAX)
    return fail(OMK_EUNSUPPORTED, "sample_rows: the edit list of a row holds %lld entries, edit_cap is %lld", (long long)SAMPLE_EDIT_MAX, (long long)p->edit_cap);
  a.edit_ids = (const int64_t*)p->edit_ids; a.edit_vals = (const float*)p->edit_vals; a.edit_lens = (const int*)p->edit_lens;
  a.edit_mode = (const int*)p->edit_mode; a.es = p->edit_stride; a.ecap = (int)p->edit_cap;
  pl.smem = edit_map_bytes(a.V) + (size_t)edit_lds_entries(a.ecap) * 8 + 4;
  return form;
}

extern "C" int omk_sample_rows_form(const OmkSampleRows* p) {
  SampleRowsPlan pl;
  return sample_rows_plan(p, pl);
}

extern "C" int omk_sample_rows(const OmkSampleRows* p, omk_stream stream) {
  SampleRowsPlan pl;
  const int form = sample_rows_plan(p, pl);
  if (form < 0) return form;
  if (pl.empty) return OMK_OK;
  const SampleRowsArgs& a = pl.a;
  const size_t smem = pl.smem;
  dim3 grid((unsigned)p->logits.shape[0]), block(SNT);
  const int dt = p->logits.dtype;
  if (form == OMK_SAMPLE_ROWS_PLAIN) {
    OMK_DISPATCH_DTYPE(dt, T, OMK_LAUNCH((sample_rows_kernel<T, SM_NONE>), grid, block, 0, stream, a));
  } else if (form == OMK_SAMPLE_ROWS_PENALTY) {
    OMK_DISPATCH_DTYPE(dt, T, {
      if (grant_map_lds<T, SM_PEN>(smem)) return fail(OMK_ELAUNCH, "sample_rows: cannot reserve %zu bytes of LDS for the id map", smem);
      OMK_LAUNCH((sample_rows_kernel<T, SM_PEN>), grid, block, smem, stream, a);
    });
  } else {
    OMK_DISPATCH_DTYPE(dt, T, {
      if (grant_map_lds<T, SM_EDIT>(smem)) return fail(OMK_ELAUNCH, "sample_rows: cannot reserve %zu bytes of LDS for the id map and the edit list", smem);
      OMK_LAUNCH((sample_rows_kernel<T, SM_EDIT>), grid, block, smem, stream, a);
    });
  }
  return finish_launch("sample_rows");
}

// ---- guided decoding: omk_sample_rows_masked (added under ABI 17; include/omk.h has the rule) ------------------------------------------
// THE selector of omk_sample_rows_masked: sample_rows_plan decides everything about p->rows as it always did; without a mask that is the
// whole answer.  With one, the checks of the mask, and which of the two masked instantiations takes the call: OMK_SAMPLE_ROWS_MASK when the
// base plan needs no id map, OMK_SAMPLE_ROWS_EDIT_MASK otherwise (the base plan's history and list, either may be absent).
static int sample_rows_masked_plan(const OmkSampleRowsMasked* p, SampleRowsPlan& pl) {
  OMK_REQUIRE(p, "sample_rows_masked: no arguments");
  const int base = sample_rows_plan(&p->rows, pl);
  if (base < 0 || !p->mask) return base;
  const int form = base == OMK_SAMPLE_ROWS_PLAIN ? OMK_SAMPLE_ROWS_MASK : OMK_SAMPLE_ROWS_EDIT_MASK;
  OMK_REQUIRE(p->mask_words >= 0 && p->mask_stride >= 0, "sample_rows_masked: mask_words and mask_stride must not be negative");
  if (pl.empty) return form;
  SampleRowsArgs& a = pl.a;
  OMK_REQUIRE(p->mask_words >= (int64_t)mask_lds_words(a.V), "sample_rows_masked: mask_words %lld holds fewer than the %d tokens of the vocabulary",
              (long long)p->mask_words, a.V);
  OMK_REQUIRE(p->rows.logits.shape[0] <= 1 || p->mask_stride >= p->mask_words, "sample_rows_masked: mask_stride %lld is below mask_words %lld",
              (long long)p->mask_stride, (long long)p->mask_words);
  if (a.V > SAMPLE_PEN_MAX_V)
    return fail(OMK_EUNSUPPORTED, "sample_rows_masked: the sampler keeps the mask of at most %lld tokens in LDS, the vocabulary has %d", (long long)SAMPLE_PEN_MAX_V, a.V);
  a.mask = (const uint32_t*)p->mask; a.mask_on = (const int*)p->mask_on; a.ms = p->mask_stride;
  const size_t mask_bytes = (size_t)mask_lds_words(a.V) * 4;
  if (form == OMK_SAMPLE_ROWS_MASK) { pl.smem = mask_bytes; return form; }
  // (a penalty launch becomes the edit layout with an empty list: a.ecap is 0 there, and the plan left the edit arrays NULL)
  pl.smem = edit_map_bytes(a.V) + (size_t)edit_lds_entries(a.ecap) * 8 + 4 + mask_bytes;
  return form;
}

extern "C" int omk_sample_rows_masked_form(const OmkSampleRowsMasked* p) {
  SampleRowsPlan pl;
  return sample_rows_masked_plan(p, pl);
}

extern "C" int omk_sample_rows_masked(const OmkSampleRowsMasked* p, omk_stream stream) {
  if (p && !p->mask) return omk_sample_rows(&p->rows, stream);   // no mask: the call IS omk_sample_rows
  SampleRowsPlan pl;
  const int form = sample_rows_masked_plan(p, pl);
  if (form < 0) return form;
  if (pl.empty) return OMK_OK;
  const SampleRowsArgs& a = pl.a;
  const size_t smem = pl.smem;
  dim3 grid((unsigned)p->rows.logits.shape[0]), block(SNT);
  const int dt = p->rows.logits.dtype;
  if (form == OMK_SAMPLE_ROWS_MASK) {
    // (at most 8 192 B of dynamic LDS: inside what every kernel may ask for without a grant)
    OMK_DISPATCH_DTYPE(dt, T, OMK_LAUNCH((sample_rows_kernel<T, SM_MASK>), grid, block, smem, stream, a));
  } else {
    OMK_DISPATCH_DTYPE(dt, T, {
      if (grant_map_lds<T, SM_EDIT_MASK>(smem)) return fail(OMK_ELAUNCH, "sample_rows_masked: cannot reserve %zu bytes of LDS for the id map, the edit list and the mask", smem);
      OMK_LAUNCH((sample_rows_kernel<T, SM_EDIT_MASK>), grid, block, smem, stream, a);
    });
  }
  return finish_launch("sample_rows_masked");
}
