// token_logprobs.hip -- log-probabilities behind the sampler (omk_token_logprobs, ABI 15; include/omk.h has the definitions): per row
// of logits the log-probability of one given token, that token's rank, and the top_n most likely tokens with their log-probabilities, all
// of the RAW row.  A launch of its own, issued only when log-probabilities are asked for: the sampler kernels (sample.hip) are not touched.
//
// One workgroup per row, as the sampler.  A row of up to TL_RV x TNT tokens (61 440 with 1024 threads: the MMU vocabulary is 50 288) is
// read from memory ONCE, every thread keeping its tokens tid, tid + TNT, ... in registers (all of a thread's loads are in flight together:
// a pass of the sampler over a row from L2 is 13 dependent rounds of 4 loads, ~7 us); the passes below then run on registers.  A longer
// row takes the same passes over memory, four requests in flight per lane, as the sampler's.
//   1. row maximum m
//   2. sum of exp(x - m), and the number of tokens in front of the given one in the order (value descending, index ascending).  Fixed order of
//      the sum: a thread adds its tokens in index order, the 64 lanes of a wave are added by the wave scan, the waves in wave order -- the
//      same in both forms of the kernel, for any row index and batch size.
//   3. top_n > 0: the sampler's 4-pass 8-bit radix select over order-preserving integer keys (eight copies of every counter in LDS), the
//      candidates gathered into LDS (ties at the threshold in index order), sorted by one wave (bitonic, ties by index).
// fkey / key_f32, the LDS add, the ballot and wave_find_digit are sample_select.h's, shared with sample.hip.  The radix select loop, the
// walk over the ties and the bitonic sort below repeat sample.hip's on keys instead of floats: moved into that header each of them changed
// this kernel's instruction sequence (the select its registers too: profiles/sampler_one_body.txt section 2).  A change to one belongs in
// the other.
#include "sample_select.h"

namespace omk {
namespace {

constexpr int TL_NMAX = SELECT_NMAX;   // = SAMPLE_KMAX of sample.hip
// threads per row: 1024, and 256 under the CPU emulator, as the sampler (the emulator executes the lanes one after the other)
#ifdef OMK_EMU
constexpr int TNT = 256;
#else
constexpr int TNT = 1024;
#endif
constexpr int TNW = TNT / 64;
constexpr int TL_RV = 60;     // tokens of the row a thread keeps in registers (REG instantiations): no scratch at 60; 50 - 56 and 64 spill
constexpr float LN2 = 0.6931471805599453f;

struct TokLpArgs {
  const void* logits; int64_t ls; int V;
  const int64_t* ids; const int* active;
  float* logprob; int64_t lps;
  int* rank; int64_t rks;
  int64_t* top_ids; int64_t tis0, tis1;
  float* top_lp; int64_t tls0, tls1;
  int top_n;
};

// REG: V <= TL_RV x TNT, the row lives in registers after one read.
template <class T, bool REG>
__global__ __launch_bounds__(TNT) void token_logprobs_kernel(TokLpArgs a) {
  // eight copies of every counter, picked by the lane (copy c of digit d at 8 d + c: see sample.hip)
  __shared__ uint32_t hist[256 * 8];
  __shared__ uint32_t sel_prefix, sel_need, n_gt, n_eq;
  __shared__ uint32_t ckey[TL_NMAX];
  __shared__ int cidx[TL_NMAX];
  __shared__ float wsum[TNW];
  __shared__ uint32_t wmax[TNW], wcnt[TNW];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.active && a.active[row] == 0) return;   // (uniform over the workgroup, in front of every barrier)
  const int V = a.V;
  const T* rowp = (const T*)a.logits + (int64_t)row * a.ls;
  // the token to score.  Nothing in ids is trusted: only an id inside the row is ever used as an index
  const int64_t id64 = a.ids ? a.ids[row] : -1;
  const bool id_ok = id64 >= 0 && id64 < (int64_t)V;
  const int id = id_ok ? (int)id64 : 0;
  const float xid = id_ok ? to_f32(rowp[id]) : NAN;
  // REG: the row as order-preserving keys, the one form every pass can use (a float is two operations away: key_f32).  The keys are made
  // opaque: a compiler that knows them to be functions of the loaded floats keeps both alive across the passes, 128 registers and scratch.
  uint32_t x[REG ? TL_RV : 1];
  if constexpr (REG) {
#pragma unroll
    for (int u = 0; u < TL_RV; u++) { const int i = tid + u * TNT; x[u] = fkey(to_f32(rowp[i < V ? i : V - 1])); }
#pragma unroll
    for (int u = 0; u < TL_RV; u++) OMK_OPAQUE(x[u]);
  }
  // one pass over the row: thread t sees the keys of its tokens t, t + TNT, ... in index order
  auto pass = [&](auto&& fn) OMK_ALWAYS_INLINE_LAMBDA {
    if constexpr (REG) {
#pragma unroll
      for (int u = 0; u < TL_RV; u++) { const int i = tid + u * TNT; if (i < V) fn(x[u], i); }
    } else {
      for (int i0 = tid; i0 < V; i0 += 4 * TNT) {
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = i0 + u * TNT; v[u] = fkey(to_f32(rowp[i < V ? i : V - 1])); }
#pragma unroll
        for (int u = 0; u < 4; u++) { const int i = i0 + u * TNT; if (i < V) fn(v[u], i); }
      }
    }
  };

  // ---- 1. row maximum
  uint32_t mk = 0u;
  pass([&](uint32_t k, int) { mk = k > mk ? k : mk; });
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const uint32_t o = shfl_xor(mk, off); mk = o > mk ? o : mk; }
  if (lane == 0) wmax[wv] = mk;
  block_sync();
  mk = wmax[0];
  for (int k = 1; k < TNW; k++) mk = wmax[k] > mk ? wmax[k] : mk;
  const float m = key_f32(mk);

  // ---- 2. sum of exp(x - m); tokens in front of the given one
  const uint32_t kid = fkey(xid);
  float s = 0.f;
  uint32_t cnt = 0u;
  pass([&](uint32_t k, int i) {
    s += exp2_fast((key_f32(k) - m) * LOG2E);
    cnt += (k > kid || (k == kid && i < id)) ? 1u : 0u;
  });
  s = wave_sum(s);
  cnt = wave_sum(cnt);
  if (lane == 0) { wsum[wv] = s; wcnt[wv] = cnt; }
  block_sync();
  s = wsum[0]; cnt = wcnt[0];
  for (int k = 1; k < TNW; k++) { s += wsum[k]; cnt += wcnt[k]; }
  const float lse = m + log2_fast(s) * LN2;
  if (tid == 0 && a.ids) {
    a.logprob[(int64_t)row * a.lps] = id_ok ? xid - lse : NAN;
    if (a.rank) a.rank[(int64_t)row * a.rks] = id_ok ? (int)(cnt + 1u) : 0;
  }
  if (a.top_n == 0) return;

  // ---- 3. radix select: the key of the K-th largest logit, 8 bits per pass from the top
  const int K = a.top_n < V ? a.top_n : V;
  if (tid == 0) { sel_prefix = 0u; sel_need = (uint32_t)K; }
  for (int ps = 0; ps < 4; ps++) {
    const int shift = 24 - 8 * ps;
    for (int i = tid; i < 256 * 8; i += TNT) hist[i] = 0u;
    block_sync();
    const uint32_t pre = sel_prefix, pmask = ps == 0 ? 0u : (0xffffffffu << (shift + 8));
    pass([&](uint32_t k, int) {
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
  pass([&](uint32_t k, int i) {
    if (k > kth) { const uint32_t sl = lds_fetch_add_u32(&n_gt, 1u); if (sl < base_eq) { ckey[sl] = k; cidx[sl] = i; } }
    else if (k == kth) { const uint32_t sl = lds_fetch_add_u32(&n_eq, 1u); if (sl < take_eq) { ckey[base_eq + sl] = k; cidx[base_eq + sl] = i; } }
  });
  block_sync();
  if (wv != 0) return;
  if (n_eq > take_eq) {
    // more logits equal the threshold than there are slots left (16-bit logits tie often): the first take_eq of them in index order are
    // the candidates, whatever order the tickets were handed out in -- one wave walks the row from memory in index order
    uint32_t got = 0u;
    for (int i0 = 0; i0 < V && got < take_eq; i0 += 64) {
      const int i = i0 + lane;
      const bool eq = i < V && fkey(to_f32(rowp[i < V ? i : V - 1])) == kth;
      const unsigned long long bm = ballot64(eq);
      const uint32_t rk = got + (uint32_t)__builtin_popcountll(bm & ((1ull << lane) - 1ull));
      if (eq && rk < take_eq) { ckey[base_eq + rk] = kth; cidx[base_eq + rk] = i; }
      got += (uint32_t)__builtin_popcountll(bm);
    }
  }
  wave_lds_sync();
  // ---- one wave: sort the K candidates (key descending, index ascending) and write them out
  uint32_t k = lane < K ? ckey[lane] : 0u;
  int ix = lane < K ? cidx[lane] : 0x7fffffff;
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      const uint32_t ok = shfl_xor(k, stride); const int oi = shfl_xor(ix, stride);
      const bool first = (lane & stride) == 0;                  // lower lane of the pair
      const bool desc = (lane & size) == 0;                     // direction of this bitonic block
      const bool mine_before = k > ok || (k == ok && ix < oi);  // "mine sorts before the other" in descending order
      const bool keep = (first == desc) ? mine_before : !mine_before;
      if (!keep) { k = ok; ix = oi; }
    }
  if (lane < a.top_n) {   // (entries past the vocabulary: id -1, log-probability -inf)
    a.top_ids[(int64_t)row * a.tis0 + (int64_t)lane * a.tis1] = lane < K ? (int64_t)ix : -1ll;
    a.top_lp[(int64_t)row * a.tls0 + (int64_t)lane * a.tls1] = lane < K ? key_f32(k) - lse : -INFINITY;
  }
}

}  // namespace
}  // namespace omk

using namespace omk;

extern "C" int omk_token_logprobs(const OmkTokenLogprobs* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->logits), "token_logprobs: logits required");
  OMK_REQUIRE(p->logits.ndim == 2 && p->logits.stride[1] == 1, "token_logprobs: logits must be (rows, vocab) with unit last stride");
  OMK_REQUIRE(p->logits.dtype == OMK_F32 || p->logits.dtype == OMK_BF16 || p->logits.dtype == OMK_F16, "token_logprobs: logits dtype");
  OMK_REQUIRE(p->top_n >= 0 && p->top_n <= TL_NMAX, "token_logprobs: top_n must be in [0, %d]", TL_NMAX);
  OMK_REQUIRE(p->ids || p->top_n > 0, "token_logprobs: nothing to do: give ids, top_n > 0 or both");
  const int64_t rows = p->logits.shape[0];
  if (p->ids) {
    OMK_REQUIRE(present(p->logprob) && p->logprob.dtype == OMK_F32 && p->logprob.ndim == 1 && p->logprob.shape[0] == rows,
                "token_logprobs: with ids, logprob must be f32 (rows)");
    OMK_REQUIRE(!present(p->rank) || (p->rank.dtype == OMK_I32 && p->rank.ndim == 1 && p->rank.shape[0] == rows), "token_logprobs: rank must be int32 (rows)");
  }
  if (p->top_n > 0) {
    OMK_REQUIRE(present(p->top_ids) && p->top_ids.ndim == 2 && p->top_ids.shape[0] == rows && p->top_ids.shape[1] == p->top_n,
                "token_logprobs: top_ids must be int64 (rows, top_n)");
    OMK_REQUIRE(present(p->top_logprobs) && p->top_logprobs.dtype == OMK_F32 && p->top_logprobs.ndim == 2 && p->top_logprobs.shape[0] == rows &&
                p->top_logprobs.shape[1] == p->top_n, "token_logprobs: top_logprobs must be f32 (rows, top_n)");
  }
  if (rows == 0) return OMK_OK;
  OMK_REQUIRE(p->logits.shape[1] > 0 && p->logits.shape[1] < (1ll << 31), "token_logprobs: vocabulary size");
  TokLpArgs a = {};
  a.logits = p->logits.data; a.ls = p->logits.stride[0]; a.V = (int)p->logits.shape[1];
  a.ids = (const int64_t*)p->ids; a.active = (const int*)p->active; a.top_n = p->top_n;
  if (p->ids) {
    a.logprob = (float*)p->logprob.data; a.lps = p->logprob.stride[0];
    a.rank = (int*)p->rank.data; a.rks = p->rank.stride[0];
  }
  if (p->top_n > 0) {
    a.top_ids = (int64_t*)p->top_ids.data; a.tis0 = p->top_ids.stride[0]; a.tis1 = p->top_ids.stride[1];
    a.top_lp = (float*)p->top_logprobs.data; a.tls0 = p->top_logprobs.stride[0]; a.tls1 = p->top_logprobs.stride[1];
  }
  dim3 grid((unsigned)rows), block(TNT);
  const int dt = p->logits.dtype;
  if (a.V <= TL_RV * TNT) OMK_DISPATCH_DTYPE(dt, T, OMK_LAUNCH((token_logprobs_kernel<T, true>), grid, block, 0, stream, a));
  else OMK_DISPATCH_DTYPE(dt, T, OMK_LAUNCH((token_logprobs_kernel<T, false>), grid, block, 0, stream, a));
  return finish_launch("token_logprobs");
}
