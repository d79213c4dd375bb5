// bksort.inc — ORDER BY ... LIMIT top-N selection for gfx950, included into
// bkgpu.hip (shares the device helpers, pool and error plumbing).
//
// Reference semantics: SortNode drains its child and emits the limit-N
// smallest rows under MemRowCompare order (src/exec/sort_node.cpp:278-440,
// src/mem_row/mem_row_compare.cpp:18-40), with ties broken by arrival index
// (TopNSorter, include/runtime/topn_sorter.h:46-54).
//
// MI355X-first design: selection, not sorting. Each row's order key is the
// composite of its order columns' order-preserving 64-bit encodings
// (bk_keyenc.h; DESC inverts bits) followed by the row id (the arrival-index
// tie-break) — a W+1-word big-endian integer with a UNIQUE value per row.
// The limit-th smallest composite is found by MSB byte-radix refinement:
//   1. one streaming scan histograms the most significant byte (filter
//      applied inline);
//   2. rows equal to the selected byte prefix are compacted into a small
//      candidate array (~n/256) which is refined byte by byte;
//   3. once the exact threshold prefix is known, one more streaming scan
//      collects rows strictly below it, the refined candidates supply the
//      remainder, and only those <= limit survivors are fully sorted
//      (LSD over words, rocPRIM radix passes — the only library primitive
//      used, on the cold <=limit-sized tail, never on the stream).
// Whole-stream work is therefore ~3 filtered scans of the order columns —
// HBM-bandwidth-bound — independent of limit.
//
// Nullable order columns are supported via marker words (below); a
// nullable FIRST order column makes word 0 a marker, which falls back to
// the scalar per-row load path in the scans.

#define TOPK_MAX_ORDER 4
#define TOPK_MAX_WORDS (2 * TOPK_MAX_ORDER + 1)

/* Composite word descriptors. A NULLable order column contributes TWO
 * words: a marker word ordering NULLs against values (is_null_first decides
 * regardless of asc/desc — mem_row_compare.cpp:22-31) followed by the value
 * word (0 for NULL rows). Non-null columns contribute one value word; the
 * final word is the rowid (arrival-order tie-break). */
#define TOPK_W_VALUE  0
#define TOPK_W_MARKER 1
#define TOPK_W_ROWID  2

/* ALL fields are per-WORD so every device access indexes by the statically
 * unrolled word id: a runtime cross-index (cols[colof[w]]) forces the
 * kernarg struct into per-lane scratch, re-read every row. */
struct TopkSpec {
    int32_t norder;
    int32_t W;                         /* total composite words incl rowid */
    int8_t  kind[TOPK_MAX_WORDS];      /* TOPK_W_* */
    int8_t  wcol[TOPK_MAX_WORDS];      /* source column of this word */
    int8_t  wasc[TOPK_MAX_WORDS];      /* ASC of this word's order col */
    int8_t  wnf[TOPK_MAX_WORDS];       /* null_first of this word's col */
};

struct Pref8 { uint64_t w[TOPK_MAX_WORDS]; };

/* Per-WORD column descriptors. `cols.c[ts.wcol[w]]` — a RUNTIME index into
 * the DevCols kernarg array — forced the whole struct into a per-lane
 * scratch copy re-read every row (measured: 3.6 KB/lane scratch, occupancy
 * 3/8, the scan at 1.5 TB/s against a ~6 TB/s streaming ceiling). With the
 * host pre-gathering one DevCol per composite word, every device access
 * indexes by the statically unrolled word id. */
struct TopkDevCols { DevCol c[TOPK_MAX_WORDS]; };

/* composite word j of row r */
__device__ __forceinline__ uint64_t topk_word(const TopkDevCols& cols,
                                              const TopkSpec& ts, int64_t r,
                                              int w) {
    int kind = ts.kind[w];
    if (kind == TOPK_W_ROWID) return (uint64_t)r;
    const DevCol& c = cols.c[w];
    if (kind == TOPK_W_MARKER) {
        bool valid = cell_valid(c, r);
        /* null_first: NULL(0) < value(1); null_last: value(0) < NULL(1) */
        return (uint64_t)(ts.wnf[w] ? (valid ? 1 : 0) : (valid ? 0 : 1));
    }
    if (c.valid && !c.valid[r]) return 0;   /* NULL value word is constant */
    uint64_t e = enc_value(c, r);
    return ts.wasc[w] ? e : ~e;
}

/* lexicographic compare of the first `nbytes` bytes of the composite of row
 * r against prefix words: -1 below, 0 equal, +1 above. w0 = the caller's
 * already-loaded word 0 (the hot column). */
/* pref word 0 arrives as a SCALAR (pref0) and the full prefix as a DEVICE
 * pointer (prefd): a pointer to (or by-value copy of) a kernarg struct
 * array forces a 64-196 B per-lane scratch copy that is re-read EVERY ROW
 * (measured on this kernel). The <= 8-byte fast path — every scan of a
 * selection that resolves within the hot word — never touches prefd. */
__device__ __forceinline__ int topk_cmp_prefix(const TopkDevCols& cols,
                                               const TopkSpec& ts, int64_t r,
                                               uint64_t pref0,
                                               const uint64_t* prefd,
                                               int nbytes, uint64_t w0) {
    if (nbytes <= 8) {   /* the common case: prefix within word 0 */
        uint64_t mask = nbytes == 8 ? ~0ull : (~0ull << (8 * (8 - nbytes)));
        uint64_t v = w0 & mask, pv = pref0 & mask;
        return v < pv ? -1 : (v > pv ? 1 : 0);
    }
    int res = 0;
    int rem = nbytes;
    #pragma unroll
    for (int w = 0; w < TOPK_MAX_WORDS; w++) {
        if (res == 0 && rem > 0 && w < ts.W) {
            int nb = rem >= 8 ? 8 : rem;
            uint64_t mask = nb == 8 ? ~0ull : (~0ull << (8 * (8 - nb)));
            uint64_t v = (w == 0 ? w0 : topk_word(cols, ts, r, w)) & mask;
            uint64_t pv = (w == 0 ? pref0 : prefd[w]) & mask;
            res = v < pv ? -1 : (v > pv ? 1 : 0);
            rem -= nb;
        }
    }
    return res;
}

#define TOPK_HISTO 0
#define TOPK_COLLECT_EQ 1
#define TOPK_COLLECT_LT 2
#define TOPK_COLLECT_BOTH 3   /* one scan fills the == prefix candidates AND
                                 the strictly-below set (two LDS stages) —
                                 replaces the separate COLLECT_EQ +
                                 COLLECT_LT full-stream passes */

/* Staged word-0 loads: the TK consecutive rows' ORDER-ENCODED word 0 via
 * back-to-back vector loads (the dhisto/dscatter whole-tile lesson — the
 * branchless per-row 8-B overlapping cell_i64 loads re-fetch each 64-B
 * line up to ~4x from HBM at 8 waves/CU; this scan measured 1.5 TB/s
 * against the ~6 TB/s streaming ceiling before staging). Width/type
 * branches are launch-uniform. Caller guarantees kind[0]==TOPK_W_VALUE
 * (a marker word 0 = nullable first order column -> scalar fallback) and
 * rb..rb+TK-1 in range (16-B column tail pad covers the vector tail). */
template <int TK>
__device__ __forceinline__ void topk_stage_w0(const DevCol& c, int8_t asc,
                                              int64_t rb, uint64_t* out) {
    static_assert(TK == 4 || TK == 8, "TK");
    const char* p = (const char*)c.data + (rb << c.lshift);
    uint64_t raw[TK];
    if (c.lshift == 3) {
        #pragma unroll
        for (int i = 0; i < TK / 2; i++)
            __builtin_memcpy(&raw[2 * i], p + 16 * i, 16);
        if (c.type == BK_DOUBLE) {
            #pragma unroll
            for (int j = 0; j < TK; j++) {
                double d;
                __builtin_memcpy(&d, &raw[j], 8);
                uint64_t e = bk_enc_f64(d);
                out[j] = asc ? e : ~e;
            }
            return;
        }
    } else if (c.lshift == 2) {
        uint64_t w[TK / 2];
        if (TK == 8) {
            #pragma unroll
            for (int i = 0; i < 2; i++)
                __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        } else {
            __builtin_memcpy(w, p, 16);
        }
        #pragma unroll
        for (int j = 0; j < TK; j++) raw[j] = w[j >> 1] >> ((j & 1) * 32);
    } else if (c.lshift == 1) {
        uint64_t w[TK == 8 ? 2 : 1];
        __builtin_memcpy(w, p, TK == 8 ? 16 : 8);
        #pragma unroll
        for (int j = 0; j < TK; j++) raw[j] = w[j >> 2] >> ((j & 3) * 16);
    } else {
        uint64_t w = 0;
        __builtin_memcpy(&w, p, TK == 8 ? 8 : 4);
        #pragma unroll
        for (int j = 0; j < TK; j++) raw[j] = w >> (j * 8);
    }
    /* INT64/DATETIME: frame-of-reference decode then sign-bit flip
     * (bk_enc_i64); STRING: dict code passes through zero-extended —
     * bit-identical to enc_value() per row */
    uint64_t flip = c.type == BK_STRING ? 0 : (1ull << 63);
    #pragma unroll
    for (int j = 0; j < TK; j++) {
        uint64_t e = ((uint64_t)c.base + (raw[j] & c.mask)) ^ flip;
        out[j] = asc ? e : ~e;
    }
}

/* one streaming pass over the rows. mode:
 *  HISTO:      histogram byte `nbytes` (0-based) of rows == prefix[0:nbytes)
 *  COLLECT_EQ: append composite entries of rows == prefix[0:nbytes)
 *  COLLECT_LT: append entries of rows < prefix[0:nbytes)                  */
/* HISTO mode histograms ALL EIGHT bytes of the word containing position
 * `nbytes` in one scan (8 x 256 bins) — leading bytes that are constant
 * across the data (e.g. uniform [0,2^31) int64 keys share their top 33
 * bits) are then consumed without extra scans. */
/* TK = rows per lane per iteration (eager word-0 loads = the loop's only
 * memory-level parallelism). HISTO scans use TK=8 (+9% on config5); the
 * COLLECT modes must keep TK=4 — their LDS stage flush guard reserves
 * blockDim*TK entries between barriers (1024), and TK=8 could add 2048
 * entries to a stage as small as ~1400 (W=9), overflowing it — found as a
 * reproducible HSA aperture fault by the round-1 soak (window fuzz seed
 * 900008 sub 0). */
/* CJ mode 0 (no WHERE conjuncts — the BASELINE config5 shape): the
 * DevCols/BkQuerySpec kernargs are never touched, so their per-lane
 * scratch copies vanish with them. CJ 1: SIMPLE padded row_passes (plain
 * compares, host-verified — q only ever indexed at constant offsets).
 * CJ 2: generic row_passes — eval_prog's runtime program-pool indexing
 * forces the ~3.5 KB BkQuerySpec kernarg into per-lane scratch (measured
 * 3.6 KB/lane, occupancy 3): correct for every shape, slow; the common
 * filtered sorts route through CJ 1. */
template <int TK, int CJ>
__global__ void __launch_bounds__(256)
k_topk_scan(DevCols cols, BkQuerySpec q, TopkDevCols tc, TopkSpec ts,
            int64_t row_begin,
            int64_t row_end, uint64_t pref0, const uint64_t* prefd,
            int nbytes, int mode,
            uint64_t* histo /*8*256*/, uint64_t* entries, uint64_t cap,
            uint64_t* counter, uint32_t* err, uint32_t STAGE_CAP,
            uint64_t* entries2, uint64_t cap2, uint64_t* counter2,
            uint32_t RESERVE) {
    /* dynamic LDS: histo mode uses 8x256 u32 bins; collect modes use an
     * entry staging buffer (TOPK_STAGE entries x W words) flushed in bulk —
     * per-match bumps of one global counter serialize at ~100 M/s and
     * per-match scattered stores waste lines. */
    /* ALL LDS in the one dynamic carve (a static __shared__ ahead of it
     * would misalign the u64 staging area — guide G17):
     *   lmem[0].lo = count, lmem[1] = flush base, lmem[2..] = lh / stage */
    extern __shared__ __attribute__((aligned(16))) uint64_t lmem[];
    uint32_t* lcnt = (uint32_t*)&lmem[0];        /* [0] eq/primary, [1] lt */
    uint64_t* lbase = &lmem[1];                  /* [0] primary, [1] lt */
    uint32_t* lh = (uint32_t*)&lmem[2];          /* [8][256] (histo mode) */
    uint64_t* stage = &lmem[3];                  /* staging (collect modes) */
    uint64_t* stage2 = stage + (size_t)STAGE_CAP * ts.W;  /* BOTH: lt */
    if (mode == TOPK_HISTO) {
        for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
            lh[i] = 0;
    } else if (threadIdx.x == 0) {
        lcnt[0] = 0;
        lcnt[1] = 0;
    }
    __syncthreads();
    int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    /* uniform per-block iteration count so collect flushes can barrier */
    int64_t range = row_end - row_begin;
    /* TK rows per lane per iteration: the eager w0 loads are the only
     * memory-level parallelism this loop has (the per-row histo/collect
     * work serializes the rest), so more rows in flight hide more HBM
     * latency (same lever measured on k_dedup_mat) */
    int64_t per_lane_span = gstride * TK;
    int64_t niter = (range + per_lane_span - 1) / per_lane_span;
    for (int64_t it = 0; it < niter; it++) {
      int64_t base = row_begin + it * per_lane_span
          + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * TK;
      /* eager word-0 loads for the TK rows (memory-level parallelism):
       * staged vector loads for a plain value word 0, scalar fallback for
       * marker word 0 / tail tiles */
      uint64_t w0e[TK];
      if (ts.kind[0] == TOPK_W_VALUE && base + TK <= row_end) {
          topk_stage_w0<TK>(tc.c[0], ts.wasc[0], base, w0e);
      } else {
          #pragma unroll
          for (int k = 0; k < TK; k++) {
              int64_t rk = base + k < row_end ? base + k : row_end - 1;
              if (rk < row_begin) rk = row_begin;
              w0e[k] = topk_word(tc, ts, rk, 0);
          }
      }
      #pragma unroll
      for (int k = 0; k < TK; k++) {
        int64_t r = base + k;
        bool live = r >= row_begin && r < row_end;
        if (CJ == 1 && live && !row_passes<true>(cols, q, r)) live = false;
        if (CJ == 2 && live && q.n_conjuncts > 0 && !row_passes(cols, q, r))
            live = false;
        int cmp = (live && nbytes)
            ? topk_cmp_prefix(tc, ts, r, pref0, prefd, nbytes, w0e[k]) : 0;
        if (mode == TOPK_HISTO) {
            if (!live || cmp != 0) continue;
            int hw = nbytes / 8;
            uint64_t wv = w0e[k];
            if (hw != 0) {
                #pragma unroll
                for (int w = 1; w < TOPK_MAX_WORDS; w++)  /* compile-time idx */
                    if (w == hw) wv = topk_word(tc, ts, r, w);
            }
            /* ONE wave vote on the top 4 bytes (constant leading bytes would
             * otherwise serialize same-address ds atomics) */
            uint64_t act = __ballot(1);
            int leader = __ffsll((unsigned long long)act) - 1;
            uint64_t hi = wv >> 32;
            uint64_t fhi = __shfl((unsigned long long)hi, leader, 64);
            if (__all(hi == fhi)) {
                if ((int)(threadIdx.x & 63) == leader) {
                    uint32_t n = (uint32_t)__popcll(act);
                    #pragma unroll
                    for (int b = 0; b < 4; b++)
                        atomicAdd(&lh[b * 256 + ((wv >> (8 * (7 - b))) & 0xFF)], n);
                }
                #pragma unroll
                for (int b = 4; b < 8; b++)
                    atomicAdd(&lh[b * 256 + ((wv >> (8 * (7 - b))) & 0xFF)], 1u);
            } else {
                #pragma unroll
                for (int b = 0; b < 8; b++)
                    atomicAdd(&lh[b * 256 + ((wv >> (8 * (7 - b))) & 0xFF)], 1u);
            }
        } else {
            bool want_eq = live && cmp == 0 &&
                           (mode == TOPK_COLLECT_EQ ||
                            mode == TOPK_COLLECT_BOTH);
            bool want_lt = live && cmp < 0 &&
                           (mode == TOPK_COLLECT_LT ||
                            mode == TOPK_COLLECT_BOTH);
            if (want_eq || want_lt) {
                /* single-collect modes use stage/lcnt[0]; BOTH routes lt
                 * through stage2/lcnt[1]. STAGE_CAP-RESERVE flush threshold
                 * below guarantees room. */
                int sl = (mode == TOPK_COLLECT_BOTH && want_lt) ? 1 : 0;
                uint64_t* st = sl ? stage2 : stage;
                uint32_t pos = atomicAdd(&lcnt[sl], 1u);
                st[pos] = w0e[k];
                #pragma unroll
                for (int w = 1; w < TOPK_MAX_WORDS; w++)  /* compile-time idx */
                    if (w < ts.W)
                        st[(size_t)w * STAGE_CAP + pos] =
                            topk_word(tc, ts, r, w);
            }
        }
      }
      if (mode != TOPK_HISTO) {
        /* bulk flush when either stage could overflow next tile, or at
         * end (one shared barrier decides both stages) */
        __syncthreads();
        uint32_t n = lcnt[0];
        uint32_t n2 = mode == TOPK_COLLECT_BOTH ? lcnt[1] : 0;
        uint32_t thr = STAGE_CAP - RESERVE;
        if (n > thr || n2 > thr || (it == niter - 1 && (n | n2))) {
            if (threadIdx.x == 0) {
                unsigned long long b =
                    atomicAdd((unsigned long long*)counter, (unsigned long long)n);
                if (b + n > cap) __hip_atomic_store(err, 1u, RLX, AGT);
                lbase[0] = b;
                lcnt[0] = 0;
                if (mode == TOPK_COLLECT_BOTH) {
                    unsigned long long b2 =
                        atomicAdd((unsigned long long*)counter2,
                                  (unsigned long long)n2);
                    if (b2 + n2 > cap2) __hip_atomic_store(err, 1u, RLX, AGT);
                    lbase[1] = b2;
                    lcnt[1] = 0;
                }
            }
            __syncthreads();
            uint64_t gbase = lbase[0];
            if (gbase + n <= cap) {
                for (uint32_t i = threadIdx.x; i < n * (uint32_t)ts.W;
                     i += blockDim.x) {
                    uint32_t e = i % n, w = i / n;
                    entries[(size_t)w * cap + gbase + e] =
                        stage[(size_t)w * STAGE_CAP + e];
                }
            }
            if (mode == TOPK_COLLECT_BOTH) {
                uint64_t gb2 = lbase[1];
                if (gb2 + n2 <= cap2) {
                    for (uint32_t i = threadIdx.x; i < n2 * (uint32_t)ts.W;
                         i += blockDim.x) {
                        uint32_t e = i % n2, w = i / n2;
                        entries2[(size_t)w * cap2 + gb2 + e] =
                            stage2[(size_t)w * STAGE_CAP + e];
                    }
                }
            }
            __syncthreads();
        }
      }
    }
    if (mode == TOPK_HISTO) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 8 * 256; i += blockDim.x)
            if (lh[i])
                atomicAdd((unsigned long long*)&histo[i],
                          (unsigned long long)lh[i]);
    }
}

/* histogram byte `nbytes` of candidate entries */
__global__ void k_topk_histo_cand(const uint64_t* entries, uint64_t cap,
                                  uint64_t n, int nbytes, uint64_t* histo) {
    __shared__ uint32_t lh[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    int w = nbytes / 8, b = nbytes % 8;
    uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gstride) {
        uint32_t byte = (uint32_t)((entries[(size_t)w * cap + i]
                                    >> (8 * (7 - b))) & 0xFF);
        atomicAdd(&lh[byte], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x)
        if (lh[i]) atomicAdd((unsigned long long*)&histo[i],
                             (unsigned long long)lh[i]);
}

/* keep candidates whose byte `nbytes` == want (compact into out) */
__global__ void k_topk_filter_cand(const uint64_t* in, uint64_t cap_in,
                                   uint64_t n, int nbytes, uint32_t want,
                                   int W, uint64_t* out, uint64_t cap_out,
                                   uint64_t* counter, uint64_t* below,
                                   uint64_t below_cap, uint64_t* below_ctr) {
    /* keep == want; in the fused flow (below != null) entries whose byte
     * sorts BELOW the pick append to the below set — they are final answer
     * rows that the skipped COLLECT_LT rescan would otherwise have caught */
    int w = nbytes / 8, b = nbytes % 8;
    uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gstride) {
        uint32_t byte = (uint32_t)((in[(size_t)w * cap_in + i]
                                    >> (8 * (7 - b))) & 0xFF);
        if (byte == want) {
            uint64_t j = atomicAdd((unsigned long long*)counter, 1ull);
            if (j >= cap_out) continue;
            for (int k = 0; k < W; k++)
                out[(size_t)k * cap_out + j] = in[(size_t)k * cap_in + i];
        } else if (below && byte < want) {
            uint64_t j = atomicAdd((unsigned long long*)below_ctr, 1ull);
            if (j >= below_cap) continue;
            for (int k = 0; k < W; k++)
                below[(size_t)k * below_cap + j] = in[(size_t)k * cap_in + i];
        }
    }
}

/* permute all W word-planes by idx (after one rocPRIM key sort pass) */
__global__ void k_topk_permute(const uint64_t* in, uint64_t cap_in,
                               const uint32_t* idx, uint64_t n, int W,
                               uint64_t* out, uint64_t cap_out) {
    uint64_t gstride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gstride)
        for (int w = 0; w < W; w++)
            out[(size_t)w * cap_out + i] = in[(size_t)w * cap_in + idx[i]];
}

static float g_topk_ms = 0.f;
extern "C" double bkgpu_topk_kernel_ms(void) { return g_topk_ms; }

/* stable LSD sort of `n` entries (SoA word planes, capacity cap) by the
 * composite (word 0 most significant). Ping-pongs between buf and tmp;
 * returns pointer holding the sorted data (== buf or tmp), or nullptr with
 * g_err set. */
static uint64_t* topk_lsd_sort(uint64_t* buf, uint64_t* tmp, uint64_t cap,
                               uint64_t n, int W) {
    if (n <= 1) return buf;
    PoolBufs bufs;
    uint32_t *idx_in = nullptr, *idx_out = nullptr;
    uint64_t* keys_out = nullptr;
    BK_TRY("topk sort", bufs.get(&idx_in, n * 4), nullptr);
    BK_TRY("topk sort", bufs.get(&idx_out, n * 4), nullptr);
    BK_TRY("topk sort", bufs.get(&keys_out, n * 8), nullptr);
    uint64_t* cur = buf;
    uint64_t* oth = tmp;
    for (int w = W - 1; w >= 0; w--) {  /* least significant word first */
        dev_iota(idx_in, n, 256);
        BK_TRY("topk sort", dev_sort_pairs(bufs, cur + (size_t)w * cap, keys_out,
                                           idx_in, idx_out, n, 0, 64), nullptr);
        hipLaunchKernelGGL(k_topk_permute, dim3(256), dim3(256), 0, 0,
                           cur, cap, idx_out, n, W, oth, cap);
        std::swap(cur, oth);
    }
    return cur;
}

extern "C" int64_t bkgpu_sort_topk(BkgTable* t, const BkQuerySpec* q,
                                   const BkOrderSpec* order, int norder,
                                   int64_t row_begin, int64_t row_end,
                                   int64_t limit, int64_t* out_rows) {
    if (t && q && query_exprs_check(t, q) != 0) return -1;
    if (ensure_device() != 0) return -1;
    if (norder < 1 || norder > TOPK_MAX_ORDER) { set_err("bad norder"); return -1; }
    if (limit <= 0) return 0;
    TopkSpec ts{};
    ts.norder = norder;
    int w = 0;
    for (int j = 0; j < norder; j++) {
        if (t->valid[order[j].col]) {       /* nullable: marker word first */
            ts.kind[w] = TOPK_W_MARKER;
            ts.wcol[w] = (int8_t)order[j].col;
            ts.wasc[w] = (int8_t)order[j].is_asc;
            ts.wnf[w] = (int8_t)order[j].is_null_first;
            w++;
        }
        ts.kind[w] = TOPK_W_VALUE;
        ts.wcol[w] = (int8_t)order[j].col;
        ts.wasc[w] = (int8_t)order[j].is_asc;
        ts.wnf[w] = (int8_t)order[j].is_null_first;
        w++;
    }
    ts.kind[w] = TOPK_W_ROWID;
    ts.W = w + 1;
    DevCols dc = table_cols(t);
    TopkDevCols tdc{};
    for (int j = 0; j < ts.W; j++)
        tdc.c[j] = dc.c[ts.wcol[j]];   /* rowid word: wcol 0, never read */
    const int W = ts.W;
    BkQuerySpec qpad;
    const BkQuerySpec* qk = q;
    int cjmode = 0;
    if (q->n_conjuncts > 0) {
        bool simple = query_simple(t, q) && getenv("BK_NO_SIMPLE") == nullptr;
        if (simple) { qpad = pad_simple_q(q); qk = &qpad; cjmode = 1; }
        else cjmode = 2;
    }
    auto scan8 = cjmode == 0   ? k_topk_scan<8, 0>
                 : cjmode == 1 ? k_topk_scan<8, 1>
                               : k_topk_scan<8, 2>;
    auto scan4 = cjmode == 0   ? k_topk_scan<4, 0>
                 : cjmode == 1 ? k_topk_scan<4, 1>
                               : k_topk_scan<4, 2>;
    /* LDS staging entries per block: cap the carve at ~100 KiB.
     * Fused COLLECT_BOTH (one scan fills == candidates AND the below set,
     * skipping the COLLECT_LT full-stream rescan) splits the carve in two;
     * each stage must keep blockDim*TK reserve free between flush barriers
     * (the round-1 aperture-fault lesson), so TK drops as W widens and the
     * fusion falls back to the two-pass flow for very wide composites.
     * BK_TOPK_FUSE=0 forces the two-pass flow. */
    /* Stage size trades flush frequency against OCCUPANCY, and occupancy
     * wins (measured, config5): 1088 entries (26 KB at W=3 -> 6 blocks/CU,
     * 6 waves/SIMD) runs the collect scans at 9.7 ms/step vs 12.4 at the
     * old 2048 (48 KB -> 3 blocks/CU) — the stage only ever holds ~8
     * matches per block-iteration at real selectivities, so the worst-case
     * reserve (1024 = blockDim*TK, the correctness invariant) IS the
     * stage; extra capacity just burns LDS. */
    size_t scap0 = 1024 + 64;
    if (const char* e = getenv("BK_TOPK_SCAP")) scap0 = (size_t)atoll(e);
    const uint32_t stage_cap = (uint32_t)std::max<size_t>(
        1024 + 64,
        std::min<size_t>(scap0, (100 * 1024) / ((size_t)W * 8)));
    size_t fcap0 = 1100;   /* best fused carve (3 blocks/CU): 10.6 ms —
                              still behind the small-stage two-pass flow
                              (9.7), so fusion defaults OFF: halving the
                              per-stage LDS (or doubling the carve) costs
                              more occupancy than the saved read pass */
    if (const char* e = getenv("BK_TOPK_FCAP")) fcap0 = (size_t)atoll(e);
    const uint32_t fuse_cap =
        (uint32_t)std::min<size_t>(fcap0, (50 * 1024) / ((size_t)W * 8));
    bool fuse = getenv("BK_TOPK_FUSE") && atoi(getenv("BK_TOPK_FUSE")) != 0;
    uint32_t fuse_reserve = 0;
    bool fuse_tk8 = false;
    if (fuse_cap >= 2048 + 64) { fuse_tk8 = true; fuse_reserve = 2048; }
    else if (fuse_cap >= 1024 + 64) { fuse_reserve = 1024; }
    else fuse = false;
    int64_t range = row_end - row_begin;
    if (range <= 0) return 0;

    uint64_t cand_cap = (uint64_t)std::max<int64_t>(
        4 * limit, std::min<int64_t>(range / 64 + 4096, int64_t(1) << 24));
    uint64_t out_cap = (uint64_t)limit + 256;
    uint64_t *histo = nullptr, *ctr = nullptr, *ctr2 = nullptr,
             *candA = nullptr, *candB = nullptr,
             *outbufA = nullptr, *outbufB = nullptr;
    uint32_t* err = nullptr;
    uint64_t h_host[8 * 256];
    Pref8 pref{};
    uint64_t* prefd = nullptr;   /* device copy for the >8-byte cmp path */
    int nbytes = 0;
    int64_t need = limit;
    uint64_t n_cand = 0;
    uint64_t n_below = 0, n_out = 0;
    PoolBufs bufs;
    DevEvents<2> evs;
    hipEvent_t &ev0 = evs.e[0], &ev1 = evs.e[1];

    BK_TRY("topk", bufs.get(&histo, 8 * 256 * 8), -1);
    BK_TRY("topk", bufs.get(&prefd, sizeof(Pref8)), -1);
    BK_TRY("topk", hipMemcpy(prefd, pref.w, sizeof(Pref8), hipMemcpyHostToDevice),
           -1);
    BK_TRY("topk", bufs.get(&ctr, 8), -1);
    BK_TRY("topk", bufs.get(&ctr2, 8), -1);
    BK_TRY("topk", hipMemset(ctr2, 0, 8), -1);
    BK_TRY("topk", bufs.get(&err, 4), -1);
    BK_TRY("topk", bufs.get(&candA, cand_cap * W * 8), -1);
    BK_TRY("topk", bufs.get(&candB, cand_cap * W * 8), -1);
    BK_TRY("topk", bufs.get(&outbufA, out_cap * W * 8), -1);
    BK_TRY("topk", bufs.get(&outbufB, out_cap * W * 8), -1);
    BK_TRY("topk", hipMemset(err, 0, 4), -1);
    BK_TRY("topk", evs.create(), -1);
    BK_TRY("topk", hipEventRecord(ev0), -1);

    /* ---- phase 1: streaming refinement until the == prefix set fits the
     * candidate buffer. Each scan histograms all 8 bytes of the current
     * word; constant leading bytes are consumed without rescanning. ---- */
    {
        bool collected = false;
        int64_t total = -1;   /* rows matching current prefix (unknown yet) */
        while (!collected) {
            BK_TRY("topk", hipMemset(histo, 0, 8 * 256 * 8), -1);
            hipLaunchKernelGGL(scan8, dim3(2048), dim3(256),
                               8 * 256 * 4 + 24, 0,
                               dc, *qk, tdc, ts, row_begin, row_end, pref.w[0],
                               prefd, nbytes,
                               TOPK_HISTO, histo, (uint64_t*)nullptr, 0,
                               (uint64_t*)nullptr, err, 0,
                               (uint64_t*)nullptr, 0, (uint64_t*)nullptr,
                               1024);
            BK_TRY("topk", hipGetLastError(), -1);
            BK_TRY("topk", hipMemcpy(h_host, histo, 8 * 256 * 8, hipMemcpyDeviceToHost), -1);
            int word0 = nbytes / 8;
            for (int b = nbytes % 8; b < 8; b++) {
                const uint64_t* h = h_host + (size_t)b * 256;
                uint64_t cum = 0;
                int pick = 255;
                for (int bkt = 0; bkt < 256; bkt++) {
                    if (cum + h[bkt] >= (uint64_t)need) { pick = bkt; break; }
                    cum += h[bkt];
                }
                if (total < 0) {
                    total = 0;
                    for (int bkt = 0; bkt < 256; bkt++) total += (int64_t)h[bkt];
                    if (total == 0) {            /* nothing passes the filter */
                        n_cand = 0; need = 0; collected = true; break;
                    }
                    if ((int64_t)limit >= total) {
                        /* selection trivial: everything qualifies */
                        need = total;
                    }
                }
                need -= (int64_t)cum;
                pref.w[nbytes / 8] |= ((uint64_t)pick) << (8 * (7 - nbytes % 8));
                nbytes++;
                BK_TRY("topk", hipMemcpy(prefd, pref.w, sizeof(Pref8),
                                         hipMemcpyHostToDevice), -1);
                int64_t cnt = (int64_t)h[pick];
                if ((uint64_t)cnt <= cand_cap) {
                    BK_TRY("topk", hipMemset(ctr, 0, 8), -1);
                    if (fuse) {
                        /* fused: == candidates AND the strictly-below set
                         * in ONE scan (ctr2 keeps accumulating through the
                         * phase-2 refinement's below-appends) */
                        BK_TRY("topk", hipMemset(ctr2, 0, 8), -1);
                        hipLaunchKernelGGL(
                            fuse_tk8 ? scan8 : scan4, dim3(2048), dim3(256),
                            (size_t)fuse_cap * W * 8 * 2 + 24, 0,
                            dc, *qk, tdc, ts, row_begin, row_end,
                            pref.w[0], prefd,
                            nbytes, TOPK_COLLECT_BOTH,
                            (uint64_t*)nullptr, candA, cand_cap,
                            ctr, err, fuse_cap,
                            outbufA, out_cap, ctr2, fuse_reserve);
                    } else {
                        /* two-pass flow: == candidates now, below set by a
                         * final COLLECT_LT rescan */
                        hipLaunchKernelGGL(scan4, dim3(2048), dim3(256),
                                           (size_t)stage_cap * W * 8 + 24, 0,
                                           dc, *qk, tdc, ts, row_begin,
                                           row_end, pref.w[0], prefd,
                                           nbytes, TOPK_COLLECT_EQ,
                                           (uint64_t*)nullptr, candA,
                                           cand_cap, ctr, err, stage_cap,
                                           (uint64_t*)nullptr, 0,
                                           (uint64_t*)nullptr, 1024);
                    }
                    BK_TRY("topk", hipGetLastError(), -1);
                    BK_TRY("topk", hipMemcpy(&n_cand, ctr, 8, hipMemcpyDeviceToHost), -1);
                    uint32_t e_host = 0;
                    BK_TRY("topk", hipMemcpy(&e_host, err, 4, hipMemcpyDeviceToHost), -1);
                    if (e_host) { set_err("sort_topk: candidate overflow"); return -1; }
                    collected = true;
                    break;
                }
                if (cnt == total) continue;  /* constant byte: deeper histos valid */
                total = cnt;                  /* narrowed: need a rescan */
                break;
            }
            (void)word0;
        }
    }

    /* ---- phase 2: candidate-array refinement ---- */
    while (n_cand > (uint64_t)std::max<int64_t>(need, 1) &&
           (int64_t)n_cand > (int64_t)out_cap / 2 && nbytes < 8 * W) {
        BK_TRY("topk", hipMemset(histo, 0, 256 * 8), -1);
        hipLaunchKernelGGL(k_topk_histo_cand, dim3(512), dim3(256), 0, 0,
                           candA, cand_cap, n_cand, nbytes, histo);
        BK_TRY("topk", hipGetLastError(), -1);
        BK_TRY("topk", hipMemcpy(h_host, histo, 256 * 8, hipMemcpyDeviceToHost), -1);
        uint64_t cum = 0;
        int pick = 255;
        for (int bkt = 0; bkt < 256; bkt++) {
            if (cum + h_host[bkt] >= (uint64_t)need) { pick = bkt; break; }
            cum += h_host[bkt];
        }
        need -= (int64_t)cum;
        pref.w[nbytes / 8] |= ((uint64_t)pick) << (8 * (7 - nbytes % 8));
        nbytes++;
        BK_TRY("topk", hipMemcpy(prefd, pref.w, sizeof(Pref8),
                                 hipMemcpyHostToDevice), -1);
        BK_TRY("topk", hipMemset(ctr, 0, 8), -1);
        hipLaunchKernelGGL(k_topk_filter_cand, dim3(512), dim3(256), 0, 0,
                           candA, cand_cap, n_cand, nbytes - 1, (uint32_t)pick,
                           W, candB, cand_cap, ctr,
                           fuse ? outbufA : (uint64_t*)nullptr, out_cap,
                           fuse ? ctr2 : (uint64_t*)nullptr);
        BK_TRY("topk", hipGetLastError(), -1);
        BK_TRY("topk", hipMemcpy(&n_cand, ctr, 8, hipMemcpyDeviceToHost), -1);
        std::swap(candA, candB);
    }

    /* ---- sort candidates, keep the `need` smallest ---- */
    {
        uint64_t* sorted = topk_lsd_sort(candA, candB, cand_cap, n_cand, W);
        if (!sorted) return -1;
        if (sorted != candA) std::swap(candA, candB);
        /* candA now holds sorted candidates */
    }
    if ((uint64_t)need > n_cand) need = (int64_t)n_cand;

    /* ---- the strictly-below set: already collected by the fused scan
     * (+ the refinement's below-appends); two-pass flow rescans ---- */
    if (fuse) {
        BK_TRY("topk", hipMemcpy(&n_below, ctr2, 8, hipMemcpyDeviceToHost), -1);
    } else {
        BK_TRY("topk", hipMemset(ctr, 0, 8), -1);
        hipLaunchKernelGGL(scan4, dim3(2048), dim3(256),
                           (size_t)stage_cap * W * 8 + 24, 0,
                           dc, *qk, tdc, ts, row_begin, row_end, pref.w[0],
                           prefd, nbytes,
                           TOPK_COLLECT_LT, (uint64_t*)nullptr, outbufA,
                           out_cap, ctr, err, stage_cap,
                           (uint64_t*)nullptr, 0, (uint64_t*)nullptr, 1024);
        BK_TRY("topk", hipGetLastError(), -1);
        BK_TRY("topk", hipMemcpy(&n_below, ctr, 8, hipMemcpyDeviceToHost), -1);
    }
    {
        uint32_t e_host = 0;
        BK_TRY("topk", hipMemcpy(&e_host, err, 4, hipMemcpyDeviceToHost), -1);
        if (e_host || n_below > out_cap) {
            set_err("sort_topk: below-set overflow (internal)");
            return -1;
        }
    }
    /* append the needed candidates behind the below set */
    for (int w = 0; w < W; w++) {
        BK_TRY("topk", hipMemcpy(outbufA + (size_t)w * out_cap + n_below,
                                 candA + (size_t)w * cand_cap, (size_t)need * 8,
                                 hipMemcpyDeviceToDevice), -1);
    }
    n_out = n_below + (uint64_t)need;
    if (n_out > (uint64_t)limit) n_out = (uint64_t)limit;

    /* ---- final full sort of the <= limit survivors ---- */
    uint64_t* res = topk_lsd_sort(outbufA, outbufB, out_cap, n_out, W);
    if (!res) return -1;
    BK_TRY("topk", hipEventRecord(ev1), -1);
    BK_TRY("topk", hipEventSynchronize(ev1), -1);
    BK_TRY("topk", hipEventElapsedTime(&g_topk_ms, ev0, ev1), -1);
    /* rowids are the last word plane */
    BK_TRY("topk", hipMemcpy(out_rows, res + (size_t)(W - 1) * out_cap,
                             (size_t)n_out * 8, hipMemcpyDeviceToHost), -1);
    return (int64_t)n_out;
}
