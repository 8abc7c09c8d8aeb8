// penalty_edits.hip -- presence and frequency penalties as a device-built edit list (omk_penalty_edits, ABI 17; include/omk.h has the rule).
// A launch of its own IN FRONT of the sampler: it turns every row's history into (id, delta) entries, merged with the request's own edit
// list, and omk_sample_rows applies them in its edit instantiation.  The sampler kernels (sample.hip) are not touched.
//
// One workgroup of 256 threads per row (GPU and emulator alike), nothing read from the host.  Both penalties act on the DISTINCT tokens of
// the counted range, so the kernel needs per entry of that range its token's count and whether it is the token's first occurrence.  There
// is no vocabulary-sized map and no LDS atomic: the counted ids are validated and staged as int32 in an LDS tile of 512, every thread
// keeps two entries of its own in registers and walks the tile with 16-byte reads -- all lanes read the SAME address, a broadcast, no bank
// conflict -- comparing four ids per read.  A first occurrence that no valid user entry names (the same walk over the staged user ids) gets
// its output slot from a ballot scan over the workgroup in position order.  n counted ids cost n^2 / 256 compares per thread: 1024 at the
// 512 ids a row's list can hold in the sampler.  A longer range (or user list) loops over tiles: the thread's own entries come straight
// from memory, the compared tile is staged each time -- correct for any length, sized for one tile.
#include "sample_select.h"

namespace omk {
namespace {

constexpr int PNT = 256;              // threads per row
constexpr int PNW = PNT / 64;
constexpr int PE_U = 2;               // entries of a tile a thread owns: t, t + PNT
constexpr int PE_TILE = PE_U * PNT;   // = the 512 entries of the sampler's edit list
constexpr uint32_t PE_NONE = 0xffffffffu;

struct PenEditArgs {
  const int64_t* history; const int* history_lens; const int* count_start; const float* frequency; const float* presence; const int* active;
  int64_t hs; int hcap;
  const int64_t* edit_ids; const float* edit_vals; const int* edit_lens; const int* edit_mode;
  int64_t es; int ecap;
  int64_t* out_ids; float* out_vals; int* out_lens; int* out_mode;
  int64_t os; int ocap;
  int V;
};

// -((f * c) + p) with the product and the sum rounded separately, in every build.  The library is compiled with -ffp-contract=fast, which
// lets the code generator fuse ANY multiply with an add that uses it, whatever a contract pragma says about the two: the rounded product
// is made opaque in between, so there is no such pair.  (The emulator build is compiled with -ffp-contract=off.)
__device__ __forceinline__ float penalty_delta(float f, float p, uint32_t c) {
  float m = f * (float)c;
  OMK_OPAQUE(m);
  return -(m + p);
}

__device__ __forceinline__ bool finite_f32(float f) { return (__builtin_bit_cast(uint32_t, f) & 0x7f800000u) != 0x7f800000u; }

// src[lo + t + u PNT] for the thread's PE_U entries of a tile: as int32, -1 for an id outside [0, V) or an index from n on; raw: the ids as
// they are.  The whole tile is written to buf, so what lies behind the row's end never matches a token.
__device__ __forceinline__ void stage_tile(const int64_t* src, int64_t lo, int64_t n, int V, int tid, int* buf, int (&own)[PE_U], int64_t (&raw)[PE_U]) {
#pragma unroll
  for (int u = 0; u < PE_U; u++) {
    const int64_t j = lo + tid + u * PNT;
    raw[u] = j < n ? src[j] : -1ll;
    own[u] = (raw[u] >= 0 && raw[u] < (int64_t)V) ? (int)raw[u] : -1;
    buf[tid + u * PNT] = own[u];
  }
}

// buf[0 .. len4) against the thread's entries: cnt[u] += the entries equal to own[u]; FIRST: first[u] = the lowest base + index of one.
// (own[u] == -1 matches the padding: the caller looks at valid entries only)
template <bool FIRST>
__device__ __forceinline__ void tile_match(const int* buf, int len4, const int (&own)[PE_U], uint32_t (&cnt)[PE_U], uint32_t (&first)[PE_U], uint32_t base) {
  for (int k = 0; k < len4; k += 4) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(buf + k);
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int u = 0; u < PE_U; u++) {
        const bool eq = v[e] == (uint32_t)own[u];
        cnt[u] += eq ? 1u : 0u;
        if constexpr (FIRST) { const uint32_t at = eq ? base + (uint32_t)(k + e) : PE_NONE; first[u] = at < first[u] ? at : first[u]; }
      }
  }
}

__device__ __forceinline__ int tile_len4(int64_t n, int64_t lo) {
  const int64_t len = n - lo < (int64_t)PE_TILE ? n - lo : (int64_t)PE_TILE;
  return ((int)len + 3) & ~3;
}

__global__ __launch_bounds__(PNT) void penalty_edits_kernel(PenEditArgs a) {
  __shared__ __attribute__((aligned(16))) int hbuf[PE_TILE];   // a tile of the counted range
  __shared__ __attribute__((aligned(16))) int ubuf[PE_TILE];   // a tile of the user list
  __shared__ uint32_t wtot[PE_U][PNW];
  __shared__ uint32_t wany[PNW];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // the row's entries in one round of scalar loads, the active flag among them (as sample_rows_kernel)
  int act = *(a.active ? a.active + row : a.history_lens + row);
  int hl = a.history_lens[row], cs = a.count_start[row];
  float fr = a.frequency[row], pr = a.presence[row];
  int el = a.edit_ids ? a.edit_lens[row] : 0;
  int em = a.edit_mode ? a.edit_mode[row] : 0;
  OMK_OPAQUE_S(hl); OMK_OPAQUE_S(cs); OMK_OPAQUE_S(fr); OMK_OPAQUE_S(pr); OMK_OPAQUE_S(el); OMK_OPAQUE_S(em); OMK_OPAQUE_S(act);
  if (a.active && act == 0) return;   // (uniform over the workgroup, in front of every barrier)
  hl = hl < 0 ? 0 : (hl > a.hcap ? a.hcap : hl);
  cs = cs < 0 ? 0 : (cs > hl ? hl : cs);
  el = el < 0 ? 0 : (el > a.ecap ? a.ecap : el);
  if (!finite_f32(fr)) fr = 0.f;
  if (!finite_f32(pr)) pr = 0.f;
  const int64_t n = (fr == 0.f && pr == 0.f) ? 0 : hl - cs;   // both off: nothing is counted, the user list goes out as it is
  const int n_tiles = (int)((n + PE_TILE - 1) / PE_TILE), u_tiles = (el + PE_TILE - 1) / PE_TILE;
  const int64_t* hrow = a.history + (int64_t)row * a.hs + cs;
  const int64_t* irow = a.edit_ids + (int64_t)row * a.es;
  const float* vrow = a.edit_vals + (int64_t)row * a.es;
  int64_t* oids = a.out_ids + (int64_t)row * a.os;
  float* ovals = a.out_vals + (int64_t)row * a.os;
  uint32_t none[PE_U];                // (tile_match<false> writes no first)
  int64_t raw[PE_U];
  bool hstaged = false;               // a counted range of one tile is staged once and stays

  // ---- 1. the user entries: ids as they are, the value of a valid counted id moved by its delta
  bool anyv = false;
  for (int ut = 0; ut < u_tiles; ut++) {
    int uown[PE_U];
    stage_tile(irow, (int64_t)ut * PE_TILE, el, a.V, tid, ubuf, uown, raw);
    bool ok = false;
#pragma unroll
    for (int u = 0; u < PE_U; u++) ok = ok || uown[u] >= 0;
    const bool wave_ok = ballot64(ok) != 0ull;
    anyv = anyv || wave_ok;
    uint32_t cnt[PE_U] = {};
    for (int B = 0; B < n_tiles; B++) {
      if (!(n_tiles == 1 && hstaged)) {
        int own[PE_U]; int64_t r[PE_U];
        block_sync();
        stage_tile(hrow, (int64_t)B * PE_TILE, n, a.V, tid, hbuf, own, r);
        block_sync();
        hstaged = true;
      }
      tile_match<false>(hbuf, tile_len4(n, (int64_t)B * PE_TILE), uown, cnt, none, 0u);
    }
#pragma unroll
    for (int u = 0; u < PE_U; u++) {
      const int j = ut * PE_TILE + tid + u * PNT;
      if (j < el && j < a.ocap) {
        const float v = vrow[j];
        oids[j] = raw[u];
        ovals[j] = (uown[u] >= 0 && cnt[u] > 0u) ? v + penalty_delta(fr, pr, cnt[u]) : v;
      }
    }
  }
  if (lane == 0) wany[wv] = anyv ? 1u : 0u;
  block_sync();   // (also: the user tile staged above is visible to the walk of part 2)
  bool any = false;
#pragma unroll
  for (int w = 0; w < PNW; w++) any = any || wany[w] != 0u;
  const bool allow = em == 1 && any;   // allow-only without a valid id: unconstrained

  // ---- 2. one entry per distinct counted token that no valid user entry names, in the order of first occurrence
  int64_t base = 0;                   // such tokens in the tiles in front
  if (!allow) {
    for (int A = 0; A < n_tiles; A++) {
      if ((int64_t)el + base >= (int64_t)a.ocap) break;   // nothing more fits (the same in every thread)
      int own[PE_U];
      if (n_tiles > 1) {            // the thread's entries straight from memory: the tile in LDS is whichever is compared
#pragma unroll
        for (int u = 0; u < PE_U; u++) {
          const int64_t j = (int64_t)A * PE_TILE + tid + u * PNT;
          const int64_t id = j < n ? hrow[j] : -1ll;
          own[u] = (id >= 0 && id < (int64_t)a.V) ? (int)id : -1;
        }
      } else if (hstaged) {
#pragma unroll
        for (int u = 0; u < PE_U; u++) own[u] = hbuf[tid + u * PNT];
      } else {
        stage_tile(hrow, 0, n, a.V, tid, hbuf, own, raw);
        block_sync();
        hstaged = true;
      }
      uint32_t cnt[PE_U] = {}, first[PE_U];
#pragma unroll
      for (int u = 0; u < PE_U; u++) first[u] = PE_NONE;
      for (int B = 0; B < n_tiles; B++) {
        if (n_tiles > 1) {
          int o[PE_U];
          block_sync();
          stage_tile(hrow, (int64_t)B * PE_TILE, n, a.V, tid, hbuf, o, raw);
          block_sync();
        }
        tile_match<true>(hbuf, tile_len4(n, (int64_t)B * PE_TILE), own, cnt, first, (uint32_t)B * (uint32_t)PE_TILE);
      }
      uint32_t named[PE_U] = {};
      for (int ut = 0; ut < u_tiles; ut++) {
        if (u_tiles > 1) {
          int o[PE_U];
          block_sync();
          stage_tile(irow, (int64_t)ut * PE_TILE, el, a.V, tid, ubuf, o, raw);
          block_sync();
        }
        tile_match<false>(ubuf, tile_len4(el, (int64_t)ut * PE_TILE), own, named, none, 0u);
      }
      // the slot of a first occurrence: the first occurrences in front of it, positions t + u PNT in the order (u, t)
      bool isnew[PE_U];
      uint32_t rank[PE_U];
#pragma unroll
      for (int u = 0; u < PE_U; u++) {
        const uint32_t g = (uint32_t)A * (uint32_t)PE_TILE + (uint32_t)(tid + u * PNT);
        isnew[u] = own[u] >= 0 && first[u] == g && named[u] == 0u;
        const unsigned long long bm = ballot64(isnew[u]);
        rank[u] = (uint32_t)__builtin_popcountll(bm & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[u][wv] = (uint32_t)__builtin_popcountll(bm);
      }
      block_sync();
      uint32_t tot = 0u;
#pragma unroll
      for (int u = 0; u < PE_U; u++)
#pragma unroll
        for (int w = 0; w < PNW; w++) {
          const uint32_t t = wtot[u][w];
#pragma unroll
          for (int uu = 0; uu < PE_U; uu++)
            if (u < uu || (u == uu && w < wv)) rank[uu] += t;
          tot += t;
        }
#pragma unroll
      for (int u = 0; u < PE_U; u++) {
        const int64_t slot = (int64_t)el + base + (int64_t)rank[u];
        if (isnew[u] && slot < (int64_t)a.ocap) {
          oids[slot] = (int64_t)own[u];
          ovals[slot] = penalty_delta(fr, pr, cnt[u]);
        }
      }
      base += (int64_t)tot;
      // (wtot is written again behind the barriers of the next tile's staging: n_tiles > 1 whenever there is a next tile)
    }
  }
  if (tid == 0) {
    const int64_t total = (int64_t)el + base;
    a.out_lens[row] = (int)(total < (int64_t)a.ocap ? total : (int64_t)a.ocap);
    a.out_mode[row] = allow ? 1 : 0;
  }
}

// every check of a call and the kernel arguments.  OMK_OK, or the status the call is refused with; empty: no row, nothing to launch
int penalty_edits_plan(const OmkPenaltyEdits* p, PenEditArgs& a, bool& empty) {
  OMK_REQUIRE(p, "penalty_edits: no parameters");
  OMK_REQUIRE(p->batch >= 0 && p->batch < (1ll << 31), "penalty_edits: batch");
  // (arrays of no entry have no address: the pointers of an empty batch are not looked at)
  OMK_REQUIRE(p->batch == 0 || (p->history && p->history_lens && p->count_start && p->frequency && p->presence),
              "penalty_edits: history, history_lens, count_start, frequency and presence are required device arrays");
  OMK_REQUIRE(p->batch == 0 || (p->out_ids && p->out_vals && p->out_lens && p->out_mode), "penalty_edits: out_ids, out_vals, out_lens and out_mode are required");
  OMK_REQUIRE(p->history_cap >= 0 && p->history_cap < (1ll << 31), "penalty_edits: history_cap");
  OMK_REQUIRE(p->out_cap >= 0 && p->out_cap < (1ll << 31), "penalty_edits: out_cap");
  OMK_REQUIRE(!p->edit_ids || (p->edit_vals && p->edit_lens), "penalty_edits: edit_ids needs edit_vals and edit_lens");
  OMK_REQUIRE(!p->edit_ids || (p->edit_cap >= 0 && p->edit_cap < (1ll << 31)), "penalty_edits: edit_cap");
  OMK_REQUIRE(p->vocab > 0 && p->vocab < (1ll << 31), "penalty_edits: vocabulary size");
  // rows one behind the other: a row stride below the width (or a negative one) would make rows overlap
  OMK_REQUIRE(p->batch <= 1 || p->history_stride >= p->history_cap, "penalty_edits: history_stride must be at least history_cap");
  OMK_REQUIRE(p->batch <= 1 || !p->edit_ids || p->edit_stride >= p->edit_cap, "penalty_edits: edit_stride must be at least edit_cap");
  OMK_REQUIRE(p->batch <= 1 || p->out_stride >= p->out_cap, "penalty_edits: out_stride must be at least out_cap");
  a = PenEditArgs{};
  empty = p->batch == 0;
  a.history = (const int64_t*)p->history; a.history_lens = (const int*)p->history_lens; a.count_start = (const int*)p->count_start;
  a.frequency = (const float*)p->frequency; a.presence = (const float*)p->presence; a.active = (const int*)p->active;
  a.hs = p->history_stride; a.hcap = (int)p->history_cap;
  if (p->edit_ids && p->edit_cap > 0) {
    a.edit_ids = (const int64_t*)p->edit_ids; a.edit_vals = (const float*)p->edit_vals; a.edit_lens = (const int*)p->edit_lens;
    a.edit_mode = (const int*)p->edit_mode; a.es = p->edit_stride; a.ecap = (int)p->edit_cap;
  }
  a.out_ids = (int64_t*)p->out_ids; a.out_vals = (float*)p->out_vals; a.out_lens = (int*)p->out_lens; a.out_mode = (int*)p->out_mode;
  a.os = p->out_stride; a.ocap = (int)p->out_cap;
  a.V = (int)p->vocab;
  return OMK_OK;
}

}  // namespace
}  // namespace omk

using namespace omk;

extern "C" int omk_penalty_edits(const OmkPenaltyEdits* p, omk_stream stream) {
  PenEditArgs a;
  bool empty;
  const int rc = penalty_edits_plan(p, a, empty);
  if (rc != OMK_OK) return rc;
  if (empty) return OMK_OK;
  dim3 grid((unsigned)p->batch), block(PNT);
  OMK_LAUNCH(penalty_edits_kernel, grid, block, 0, stream, a);
  return finish_launch("penalty_edits");
}
