/* ---------------------------------------------------------------------
 * Sort-based level-1 dedup aggregate (high-cardinality DISTINCT).
 *
 * The hash path (run_partitioned + k_part_agg) degrades when the dedup
 * cardinality approaches the row count — the reference's multi-distinct
 * rewrite (agg_node.cpp:247-258) groups level 1 by (user keys + d), so
 * COUNT(DISTINCT d) over ~unique d makes #groups ~ #rows: the global
 * table regrows toward the row count and every LDS generation flushes
 * (measured 30 s at 5e8 rows / 2.3e8 dedup pairs, DESIGN.md §6).
 *
 * This path instead:
 *   1. k_dedup_mat   : predicate + spec-packed key, wave-compact
 *                      (key, rowid) pairs into dense arrays
 *   2. rocprim radix_sort_pairs on the packed key (only the declared
 *      group_bits + null-flag byte are sorted — end_bit = bits+8)
 *   3. k_dedup_heads + rocprim inclusive_scan -> dense group index per row
 *   4. k_dedup_emit  : one DENSE table slot per unique key (state=2);
 *                      per-row agg updates gather inputs by rowid
 * The dense table is a valid BkgAggOut table: compact/fetch scan slots
 * linearly, and bkgpu_agg_merge's capacity check (fill*8 > nslots*7) is
 * always true for a dense table, so any cross-rank merge first rebuilds
 * it as a regular hash table from its own blob — results identical.
 *
 * Requirements (checked; caller falls back to the hash path otherwise):
 * all group keys packed into k0 within 56 bits — via DECLARED group_bits
 * or AUTO-derived per-key spans from column stats (the null-flag byte
 * rides at bits [bits_total, bits_total+8); emit reconstructs the exact
 * spec layout either way) — and row range < 2^32 (rowids are u32).
 * Keys <= 24 bits sort as u32 (fewer radix passes); >= 2 agg inputs
 * switch to record-carrying mode (REC).
 * ------------------------------------------------------------------- */

/* internal auto-packing: when the query declares no group_bits, the host
 * derives per-key spans from column stats (ensure_stats) and the sort key
 * packs (enc - base) chunks; emit reconstructs the RAW spec layout
 * (k0 = key0 enc, k1 = key1 enc) so results are byte-identical to the hash
 * path. sp.n == 0 means declared-bits passthrough (pack_group_keys). */
struct SortPack {
    int32_t n;                 /* 0 = declared-bits mode */
    int32_t bits[2];
    uint64_t base[2];          /* encoded minima */
};

template <bool SIMPLE = false>
__device__ __forceinline__ uint64_t pack_keys_internal(
        const DevCols& cols, const BkQuerySpec& q, int64_t r,
        const SortPack& sp, int bits_total) {
    uint64_t key = 0;
    uint32_t flag = 0;
    int shift = 0;
    /* SIMPLE: the host pads sp to n == 2 (bits[1] = 0 contributes nothing,
     * group_cols[1] duplicates group_cols[0]) so the loop is branch-free
     * straight-line code — enc_value_nf instead of the type switch, no
     * early break, no validity/fn checks (query_simple guarantees). */
    #pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!SIMPLE && k >= sp.n) break;
        const DevCol& c = cols.c[q.group_cols[k]];
        if (!SIMPLE && !cell_valid(c, r)) {
            flag |= 0x80u >> k;
        } else {
            uint64_t e = SIMPLE ? enc_value_nf(c, r)
                         : q.group_fns[k]
                             ? bk_enc_i64(bk_scalar_fn(q.group_fns[k],
                                                       cell_i64(c, r)))
                             : enc_value(c, r);
            key |= ((e - sp.base[k]) & ((1ull << sp.bits[k]) - 1ull)) << shift;
        }
        shift += sp.bits[k];
    }
    return key | ((uint64_t)flag << bits_total);
}

/* pass A of the split materialize: pure predicate scan -> one ballot word
 * per 64 rows. No compaction machinery in the loop, so it runs at the
 * streaming-probe ceiling (~5.2 TB/s vs ~3.4 for the fused mat). */
template <bool SIMPLE>
__global__ void k_dedup_mask(DevCols cols, BkQuerySpec q, int64_t row_begin,
                             int64_t row_end, uint64_t* mask) {
    const int lane = threadIdx.x & 63;
    int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = row_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         ; r += gstride) {
        bool live = r < row_end;
        if (!__any(live)) break;
        bool pass = live && row_passes<SIMPLE>(cols, q, r);
        uint64_t m = __ballot(pass);
        if (lane == 0) mask[(r - row_begin) >> 6] = m;
    }
}

#ifndef BK_DEDUP_MAT_T
#define BK_DEDUP_MAT_T 16
#endif
/* KeyT: u32 when the packed key + flag byte fit 32 bits (faster radix
 * passes), u64 otherwise. REC: materialize full RecLayout records instead
 * of rowids — chosen when >= 2 agg inputs would otherwise each pay their
 * own random gather at emit (one 32 B record gather replaces them). */
template <bool SIMPLE, typename KeyT, bool REC, bool MASKED = false,
          bool SP = true>
__global__ void k_dedup_mat(DevCols cols, BkQuerySpec q, int64_t row_begin,
                            int64_t row_end, int bits_total, SortPack sp,
                            RecLayout lay, KeyT* keys,
                            uint32_t* rids, uint64_t* rec, uint64_t* ctr,
                            const uint64_t* mask = nullptr) {
    /* block-aggregated allocation with T rows per lane per round: ONE
     * global atomic and two barriers cover T*blockDim rows (a per-wave
     * atomic on the single counter serializes ~8M same-address atomics,
     * ~80 ms at 5e8 rows; per-ROW barriers lockstep the loads, ~4x the
     * streaming floor at 1e8 rows — both measured). */
    constexpr int T = BK_DEDUP_MAT_T;
    __shared__ uint32_t wbase[16];          /* per-wave exclusive prefix */
    __shared__ unsigned long long bbase;
    const int nwaves = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r0 = row_begin + (int64_t)blockIdx.x * blockDim.x
                      + threadIdx.x;
         ; r0 += gstride * T) {
        bool any = r0 < row_end;
        if (!__syncthreads_or((int)any)) break;
        KeyT key[T];
        uint32_t passbits = 0;   /* this lane's pass bit per j — phase 2
                                  * only needs (ballot >> lane) & 1, so the
                                  * T ballots don't stay in registers (they
                                  * cost 2 VGPRs each; occupancy 7 -> 4
                                  * measured as a 30% mat regression) */
        uint32_t pre[T];
        uint32_t wtot = 0;
        #pragma unroll
        for (int j = 0; j < T; j++) {
            int64_t r = r0 + (int64_t)j * gstride;
            bool pass;
            /* (an unconditional-key variant — predicate and key evaluated
             * branchlessly at a tail-clamped row, 32-deep load batches in
             * the ISA — measured SLOWER: 7.1 ms vs 5.3 at T=16, 5.4 at T=8;
             * the batching cost occupancy 7 -> 4-5 and the kernel is L1-
             * transaction-bound, not load-latency-bound. DESIGN.md §6.) */
            if (MASKED) {
                uint64_t mw = r < row_end
                                  ? mask[(uint64_t)(r - row_begin) >> 6] : 0;
                pass = r < row_end && ((mw >> lane) & 1ull);
            } else {
                pass = r < row_end && row_passes<SIMPLE>(cols, q, r);
            }
            key[j] = 0;
            if (SIMPLE && SP) {   /* compile-time: keeps the declared-bits
                                   * pack (and its enc_value type branches)
                                   * OUT of this loop entirely */
                if (pass)
                    key[j] = (KeyT)pack_keys_internal<true>(cols, q, r, sp,
                                                            bits_total);
            } else if (pass) {
                if (sp.n) {
                    key[j] = (KeyT)pack_keys_internal<SIMPLE>(cols, q, r, sp,
                                                              bits_total);
                } else {
                    KeyPack kp = pack_group_keys<SIMPLE>(cols, q, r);
                    key[j] = (KeyT)(kp.k0 |
                                    ((uint64_t)kp.flag << bits_total));
                }
            }
            uint64_t mj = __ballot(pass);
            passbits |= pass ? (1u << j) : 0u;
            pre[j] = wtot + (uint32_t)__popcll(mj & ((1ull << lane) - 1ull));
            wtot += (uint32_t)__popcll(mj);
        }
        if (lane == 0) wbase[wave] = wtot;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < nwaves; w++) {
                uint32_t c = wbase[w];
                wbase[w] = tot;
                tot += c;
            }
            bbase = tot ? atomicAdd((unsigned long long*)ctr,
                                    (unsigned long long)tot)
                        : 0ull;
        }
        __syncthreads();
        uint64_t base = bbase + wbase[wave];
        #pragma unroll
        for (int j = 0; j < T; j++) {
            if ((passbits >> j) & 1u) {
                int64_t r = r0 + (int64_t)j * gstride;
                uint64_t pos = base + pre[j];
                keys[pos] = key[j];
                if (REC) {
                    KeyPack kp = pack_group_keys<SIMPLE>(cols, q, r);
                    uint64_t regs[8];
                    build_record(cols, q, lay, r, kp, regs);
                    scatter_store_rec(rec + pos * lay.nwords, regs,
                                      lay.nwords);
                } else {
                    rids[pos] = (uint32_t)(r - row_begin);
                }
            }
        }
        __syncthreads();   /* wbase/bbase reused next round */
    }
}

/* VECTOR-LOAD materialize (SIMPLE, spec-pack, no REC, no mask): each lane
 * owns T=16 CONSECUTIVE rows; every conjunct column of physical width
 * <= 4 B (narrow u8/u16/u32 and wide string dicts) is read with ONE
 * unconditional 16-byte load per 4-row sub-chunk — 4 loads per conjunct
 * per chunk instead of 16 overlapping unaligned 8-byte decodes (the
 * L1-transaction bound DESIGN §6 names). The 16 B load covers the 4 rows
 * exactly at u32 and overreads within the chunk (u16) or up to 12 B past
 * the column at u8 — column buffers carry a 16 B tail pad for exactly
 * this. Field extraction is branchless: byte offset j << lshift never
 * straddles an 8-byte word for widths dividing 8. Output order differs
 * from the strided kernel — irrelevant: the stable radix sort that
 * follows orders by key, and per-group aggregation is order-independent
 * up to the stated double tolerance. */
/* UKEY: also vector-load the (padded-to-2) group-key columns and pack the
 * sort key UNCONDITIONALLY from registers — removes the divergent
 * dependent key gather from the pass branch so every load in the kernel
 * streams. Costs the full key column read even at low selectivity; the
 * strided unconditional-key experiment died on occupancy (32-deep scalar
 * batches), not traffic — here the key adds one 16 B load per 4 rows. */
template <typename KeyT, bool UKEY>
__global__ void __launch_bounds__(512)
k_dedup_mat_vec(DevCols cols, BkQuerySpec q, int64_t row_begin,
                int64_t row_end, int bits_total, SortPack sp,
                KeyT* keys, uint32_t* rids, uint64_t* ctr) {
    constexpr int T = 16;
    __shared__ uint32_t wbase[16];
    __shared__ unsigned long long bbase;
    const int nwaves = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    int64_t lin = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t b0 = row_begin + lin * T; ; b0 += gstride * T) {
        bool any = b0 < row_end;
        if (!__syncthreads_or((int)any)) break;
        uint32_t passbits = 0;
        KeyT key[T];
        if (b0 + T <= row_end) {
            #pragma unroll
            for (int g = 0; g < T / 4; g++) {
                int64_t rb = b0 + (int64_t)g * 4;
                uint64_t w[4][2];
                #pragma unroll
                for (int k = 0; k < 4; k++) {
                    const DevCol& c = cols.c[q.conjuncts[k].col];
                    __builtin_memcpy(w[k],
                                     (const char*)c.data + (rb << c.lshift),
                                     16);
                }
                uint64_t kw[2][2];
                if (UKEY) {
                    #pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const DevCol& c = cols.c[q.group_cols[k]];
                        __builtin_memcpy(kw[k],
                                         (const char*)c.data
                                             + (rb << c.lshift), 16);
                    }
                }
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    bool p = true;
                    #pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const BkConjunct& cj = q.conjuncts[k];
                        const DevCol& c = cols.c[cj.col];
                        unsigned off = (unsigned)j << c.lshift;  /* <= 12 */
                        uint64_t raw = (w[k][off >> 3] >> ((off & 7) * 8))
                                       & c.mask;
                        int64_t v = (int64_t)((uint64_t)c.base + raw);
                        int cmp = (v > cj.lit_i) - (v < cj.lit_i);
                        p = p & (bool)((0x19D2Au >> (3 * cj.op + cmp + 1))
                                       & 1u);
                    }
                    if (UKEY) {
                        /* branchless pack_keys_internal<true> from the
                         * vector registers (flag = 0: SIMPLE is non-null) */
                        uint64_t kv = 0;
                        int shift = 0;
                        #pragma unroll
                        for (int k = 0; k < 2; k++) {
                            const DevCol& c = cols.c[q.group_cols[k]];
                            unsigned off = (unsigned)j << c.lshift;
                            uint64_t raw = (kw[k][off >> 3]
                                            >> ((off & 7) * 8)) & c.mask;
                            uint64_t flip = c.type == BK_STRING
                                                ? 0 : (1ull << 63);
                            uint64_t e = ((uint64_t)c.base + raw) ^ flip;
                            kv |= ((e - sp.base[k])
                                   & ((1ull << sp.bits[k]) - 1ull)) << shift;
                            shift += sp.bits[k];
                        }
                        key[g * 4 + j] = (KeyT)kv;
                        passbits |= p ? 1u << (g * 4 + j) : 0u;
                    } else if (p) {
                        passbits |= 1u << (g * 4 + j);
                        key[g * 4 + j] = (KeyT)pack_keys_internal<true>(
                            cols, q, rb + j, sp, bits_total);
                    }
                }
            }
        } else {          /* tail chunk: per-row scalar, same semantics */
            #pragma unroll
            for (int j = 0; j < T; j++) {
                int64_t r = b0 + j;
                if (r < row_end && row_passes<true>(cols, q, r)) {
                    passbits |= 1u << j;
                    key[j] = (KeyT)pack_keys_internal<true>(cols, q, r, sp,
                                                            bits_total);
                }
            }
        }
        uint32_t pre[T];
        uint32_t wtot = 0;
        #pragma unroll
        for (int j = 0; j < T; j++) {
            uint64_t mj = __ballot((passbits >> j) & 1u);
            pre[j] = wtot + (uint32_t)__popcll(mj & ((1ull << lane) - 1ull));
            wtot += (uint32_t)__popcll(mj);
        }
        if (lane == 0) wbase[wave] = wtot;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w2 = 0; w2 < nwaves; w2++) {
                uint32_t c2 = wbase[w2];
                wbase[w2] = tot;
                tot += c2;
            }
            bbase = tot ? atomicAdd((unsigned long long*)ctr,
                                    (unsigned long long)tot)
                        : 0ull;
        }
        __syncthreads();
        uint64_t obase = bbase + wbase[wave];
        #pragma unroll
        for (int j = 0; j < T; j++) {
            if ((passbits >> j) & 1u) {
                uint64_t pos = obase + pre[j];
                keys[pos] = key[j];
                rids[pos] = (uint32_t)(b0 + j - row_begin);
            }
        }
        __syncthreads();
    }
}

template <typename KeyT>
__global__ void k_dedup_heads(const KeyT* keys, uint64_t n, uint32_t* f) {
    uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        f[i] = (i == 0) || (keys[i] != keys[i - 1]);
}

/* flush one locally-accumulated run into its slot: one atomic per agg word
 * per RUN instead of per row (sorted input makes same-slot runs adjacent,
 * and per-row atomics serialize ~26-deep on config2-shaped group sizes).
 * This is agg_part_fold<false> (bkgpu.hip) spelled out over the three
 * accumulator arrays, and the arms of k_dedup_emit below are
 * agg_part_of_row (and its twin over a record) spelled out: through helpers
 * k_dedup_emit<8, uint32, true> gains 20 B/lane of scratch, or the whole
 * kernel is re-allocated and measured slower. Keep them in step. */
template <int NA>
__device__ __forceinline__ void dedup_flush_run(
        uint64_t* slot, const BkQuerySpec& q, const uint64_t* accv,
        const uint64_t* accc, const double* accd) {
    #pragma unroll
    for (int32_t a = 0; a < NA; a++) {
        if (a >= q.n_aggs) break;
        uint64_t* val = slot + SLOT_HDR + 2 * a;
        uint64_t* cnt = val + 1;
        int at = q.aggs[a].agg_type;
        switch (at) {
            case BK_AGG_COUNT_STAR:
            case BK_AGG_COUNT:
                if (accv[a])
                    atomicAdd((unsigned long long*)val,
                              (unsigned long long)accv[a]);
                break;
            case BK_AGG_MIN:
            case BK_AGG_MAX:
                if (accc[a]) {
                    atomicMax((unsigned long long*)val,
                              (unsigned long long)accv[a]);
                    atomicAdd((unsigned long long*)cnt,
                              (unsigned long long)accc[a]);
                }
                break;
            default:  /* SUM / AVG */
                if (accc[a]) {
                    if (q.agg_in_types[a] == BK_DOUBLE || at == BK_AGG_AVG)
                        atomic_add_f64_global(val, accd[a]);
                    else
                        atomicAdd((unsigned long long*)val,
                                  (unsigned long long)accv[a]);
                    atomicAdd((unsigned long long*)cnt,
                              (unsigned long long)accc[a]);
                }
                break;
        }
    }
}

/* wave-cyclic emit with a shuffle-based SEGMENTED reduction: lanes hold 64
 * CONSECUTIVE sorted positions (coalesced gidx/rid loads — a per-lane
 * blocked window turns every load into a 64-line gather and ran 10x slower),
 * runs are segments, and one atomic flush happens per segment per wave
 * (~run_length/64 atomics per group instead of one per row).
 * Scan monoid over (flag, value): (f1,v1) then (f2,v2) = (f1|f2,
 * f2 ? v2 : v1 op v2) — inclusive left scan in 6 shuffle steps. */
template <int NA, typename KeyT, bool REC>
__global__ void k_dedup_emit(DevCols cols, BkQuerySpec q, int64_t row_begin,
                             int bits_total, SortPack sp, RecLayout lay,
                             const KeyT* keys,
                             const uint32_t* rids, const uint64_t* rec,
                             const uint32_t* gidx,
                             uint64_t n, uint64_t* table) {
    const int stride = SLOT_HDR + 2 * q.n_aggs;
    const int lane = threadIdx.x & 63;
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane;
         base < (int64_t)n; base += gs) {
        int64_t i = base + lane;
        bool active = i < (int64_t)n;
        uint32_t g = active ? gidx[i] : 0u;
        uint32_t gp = (uint32_t)__shfl_up((int)g, 1, 64);
        if (lane == 0) gp = (active && i > 0) ? gidx[i - 1] : ~0u;
        bool head = active && (i == 0 || gp != g);
        uint64_t* slot = active ? table + (uint64_t)(g - 1) * stride : nullptr;
        if (head) {
            /* head of the run writes the header; agg words were zeroed by
             * agg_alloc, so concurrent atomics are safe */
            uint64_t key = (uint64_t)keys[i];
            uint32_t flag = (uint32_t)(key >> bits_total);
            ((uint32_t*)slot)[0] = 2u;
            ((uint32_t*)slot)[1] = flag;
            if (sp.n) {
                /* reconstruct the RAW spec layout from packed chunks */
                uint64_t e0 = 0, e1 = 0;
                if (!(flag & 0x80u))
                    e0 = (key & ((1ull << sp.bits[0]) - 1ull)) + sp.base[0];
                if (sp.n > 1 && !(flag & 0x40u))
                    e1 = ((key >> sp.bits[0]) &
                          ((1ull << sp.bits[1]) - 1ull)) + sp.base[1];
                slot[1] = e0;
                slot[2] = e1;
            } else {
                slot[1] = bits_total >= 64
                              ? key
                              : (key & ((1ull << bits_total) - 1ull));
                slot[2] = 0;
            }
        }
        /* per-position contributions: REC mode reads the materialized
         * record (ONE 32 B gather); rid mode gathers each agg input column
         * separately */
        int64_t r = (!REC && active) ? row_begin + (int64_t)rids[i] : 0;
        uint64_t rw[8];
        uint64_t rmeta = ~0ull;
        if (REC && active) {
            const uint64_t* my = rec + (uint64_t)rids[i] * lay.nwords;
            #pragma unroll
            for (int w = 0; w < 8; w++)
                rw[w] = w < lay.nwords ? my[w] : 0;
            if (lay.meta_word >= 0) rmeta = rw[lay.meta_word];
        }
        uint64_t accv[NA];
        uint64_t accc[NA];
        double accd[NA];
        bool ismax[NA];
        #pragma unroll
        for (int32_t a = 0; a < NA; a++) {
            accv[a] = 0; accc[a] = 0; accd[a] = 0.0; ismax[a] = false;
            if (a >= q.n_aggs || !active) continue;
            const BkAggSpec& as = q.aggs[a];
            if (REC) {
                int at = as.agg_type;
                ismax[a] = (at == BK_AGG_MIN || at == BK_AGG_MAX);
                int valid = at == BK_AGG_COUNT_STAR ||
                            ((rmeta >> (8 + a)) & 1);
                if (at == BK_AGG_COUNT_STAR) { accv[a] = 1; continue; }
                if (!valid) continue;
                if (at == BK_AGG_COUNT) { accv[a] = 1; continue; }
                uint64_t w = rw[lay.val_word[a]];
                switch (at) {
                    case BK_AGG_SUM:
                        if (q.agg_in_types[a] == BK_DOUBLE)
                            memcpy(&accd[a], &w, 8);
                        else accv[a] = w;
                        accc[a] = 1;
                        break;
                    case BK_AGG_AVG:
                        memcpy(&accd[a], &w, 8);
                        accc[a] = 1;
                        break;
                    case BK_AGG_MIN: accv[a] = ~w; accc[a] = 1; break;
                    case BK_AGG_MAX: accv[a] = w;  accc[a] = 1; break;
                    default: break;
                }
                continue;
            }
            switch (as.agg_type) {
                case BK_AGG_COUNT_STAR: accv[a] = 1; break;
                case BK_AGG_COUNT:
                    accv[a] = agg_input(cols, q, as, q.agg_in_types[a], r).valid
                                  ? 1 : 0;
                    break;
                case BK_AGG_SUM: {
                    AggIn v = agg_input(cols, q, as, q.agg_in_types[a], r);
                    if (!v.valid) break;
                    if (q.agg_in_types[a] == BK_DOUBLE) accd[a] = v.d;
                    else accv[a] = (uint64_t)v.i;
                    accc[a] = 1;
                    break;
                }
                case BK_AGG_AVG: {
                    AggIn v = agg_input(cols, q, as, q.agg_in_types[a], r);
                    if (!v.valid) break;
                    accd[a] = v.d;
                    accc[a] = 1;
                    break;
                }
                case BK_AGG_MIN: {
                    ismax[a] = true;
                    AggIn v = agg_input(cols, q, as, q.agg_in_types[a], r);
                    if (!v.valid) break;
                    accv[a] = ~agg_enc(cols, as, q.agg_in_types[a], v, r);
                    accc[a] = 1;
                    break;
                }
                case BK_AGG_MAX: {
                    ismax[a] = true;
                    AggIn v = agg_input(cols, q, as, q.agg_in_types[a], r);
                    if (!v.valid) break;
                    accv[a] = agg_enc(cols, as, q.agg_in_types[a], v, r);
                    accc[a] = 1;
                    break;
                }
                default: break;
            }
        }
        /* inclusive segmented scan across the wave (inactive lanes are
         * their own empty segments so they never pollute a real run) */
        bool segf = head || !active;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            bool f_up = (bool)__shfl_up((int)segf, d, 64);
            bool take = lane >= d && !segf;
            #pragma unroll
            for (int32_t a = 0; a < NA; a++) {
                if (a >= q.n_aggs) break;
                uint64_t v_up = __shfl_up((unsigned long long)accv[a], d, 64);
                uint64_t c_up = __shfl_up((unsigned long long)accc[a], d, 64);
                double dd_up = __shfl_up(accd[a], d, 64);
                if (take) {
                    if (ismax[a]) accv[a] = v_up > accv[a] ? v_up : accv[a];
                    else accv[a] += v_up;
                    accc[a] += c_up;
                    accd[a] += dd_up;
                }
            }
            if (take) segf = f_up;
            else if (lane >= d) segf = true;  /* own-flag absorbs: boundary
                                                 found at or before here */
        }
        /* segment-last lanes flush */
        bool head_next = (bool)__shfl_down((int)head, 1, 64);
        bool active_next = (bool)__shfl_down((int)active, 1, 64);
        if (lane == 63) { head_next = true; active_next = false; }
        bool last = active && (head_next || !active_next || lane == 63);
        if (last)
            dedup_flush_run<NA>(slot, q, accv, accc, accd);
    }
}

/* Level-1 aggregate via sort-dedup. Returns nullptr with an error message
 * when the query shape does not qualify — callers fall back to
 * bkgpu_filter_agg. Results are identical to the hash path (dedup is
 * exact; int64 states bit-exact; f64 sums differ only in add order). */
extern "C" BkgAggOut* bkgpu_filter_agg_sorted(BkgTable* t, const BkQuerySpec* q,
                                              int64_t row_begin,
                                              int64_t row_end) {
    if (!t || !q || q->n_group < 1) { set_err("sorted: need GROUP BY"); return nullptr; }
    if (query_shape_check(t, q) != 0) return nullptr;
    SortPack sp{};
    const BkKeyLayout kl = bk_key_layout(q);
    int bits_total = 0;
    for (int32_t k = 0; k < kl.n; k++) bits_total += kl.bits[k];
    if (bits_total > 56) {
        /* no usable declared widths: AUTO-pack from column stats (per-key
         * encoding span; works for INT64/DATETIME/DOUBLE/dict encodings
         * alike since only exact encodings are reconstructed at emit) */
        if (q->n_group > 2) {
            set_err("sorted: auto-pack supports <= 2 group keys");
            return nullptr;
        }
        if (ensure_device() != 0) return nullptr;
        bits_total = 0;
        for (int32_t k = 0; k < q->n_group; k++) {
            if (q->group_fns[k]) {
                set_err("sorted: auto-pack cannot bound fn-key spans");
                return nullptr;
            }
            int col = q->group_cols[k];
            if (ensure_stats(t, col) != 0) return nullptr;
            uint64_t lo = t->stat_min[col], hi = t->stat_max[col];
            uint64_t span = hi >= lo ? hi - lo : 0;
            int b = span ? 64 - __builtin_clzll(span) : 1;
            sp.bits[k] = b;
            sp.base[k] = hi >= lo ? lo : 0;
            bits_total += b;
        }
        sp.n = q->n_group;
        if (bits_total > 56) {
            set_err("sorted: key spans exceed 56 packed bits");
            return nullptr;
        }
    }
    int64_t range = row_end - row_begin;
    if (range <= 0) { set_err("sorted: empty range"); return nullptr; }
    if (range >= (int64_t)UINT32_MAX) {
        set_err("sorted: range too large for one pass");
        return nullptr;
    }
    if (ensure_device() != 0) return nullptr;
    DevCols dc = table_cols(t);

    RecLayout lay;
    build_rec_layout(t, q, &lay);
    int nvals = 0;
    for (int32_t a = 0; a < q->n_aggs; a++)
        if (lay.val_word[a] >= 0) nvals++;
    /* record mode: >= 2 agg inputs -> ONE record gather at emit instead of
     * one random gather per input column */
    bool recmode = nvals >= 2 && getenv("BK_NO_REC") == nullptr;
    bool key32 = bits_total + 8 <= 32;
    size_t ksz = key32 ? 4 : 8;

    /* the emit kernel may still be in flight when bufs goes out of scope:
     * see the INVARIANT at PoolBufs */
    PoolBufs bufs;
    void *keys = nullptr, *keys2 = nullptr;
    uint64_t *ctr = nullptr, *rec = nullptr, *mask = nullptr;
    uint32_t *rids = nullptr, *rids2 = nullptr, *f = nullptr, *gidx = nullptr;
    BK_TRY("sorted", bufs.get(&keys, (size_t)range * ksz), nullptr);
    BK_TRY("sorted", bufs.get(&rids, (size_t)range * 4), nullptr);
    if (recmode)
        BK_TRY("sorted", bufs.get(&rec, (size_t)range * lay.nwords * 8), nullptr);
    BK_TRY("sorted", bufs.get(&ctr, 8), nullptr);
    BK_TRY("sorted", hipMemset(ctr, 0, 8), nullptr);

    static const char* NAMESD[] = {"dedup_mat", "sort", "scan", "emit"};
    EvTimer tm;
    tm.record();
    bool simple = query_simple(t, q) && !getenv("BK_NO_SIMPLE");
    /* SIMPLE kernels run on a PADDED query copy: conjuncts replicated to 4
     * (idempotent under AND; a GE INT64_MIN tautology when none) and sp
     * padded to 2 keys (bits[1]=0) — the phase-1 loops then compile with
     * no per-row uniform branches and the scheduler batches the loads. */
    BkQuerySpec qpad;
    SortPack sppad = sp;
    const BkQuerySpec* qk = q;
    if (simple) {
        qpad = pad_simple_q(q);
        if (sp.n == 1) {
            sppad.n = 2;
            sppad.bits[1] = 0;
            sppad.base[1] = 0;
            qpad.group_cols[1] = qpad.group_cols[0];
        }
        qk = &qpad;
    }
    int mat_blocks = 8192;
    if (const char* e = getenv("BK_MAT_BLOCKS")) mat_blocks = atoi(e);
    /* split materialize (OPT-IN, measured DEAD at defaults): a
     * predicate->bitmask pass + a mask-driven compaction pass was expected
     * to run the scan portion at the probe ceiling, but measured 6.1 ms vs
     * 4.9 for the fused mat on the 1e9-row 8-int64 shape — the mask pass
     * gains nothing over the fused loop's batched loads, so the second
     * pass's mask+key reads are pure overhead. Kept behind BK_MAT_SPLIT
     * for re-testing. */
    bool split = q->n_conjuncts > 0 && range >= 30 * 1000 * 1000 &&
                 getenv("BK_MAT_SPLIT") != nullptr;
    if (split && bufs.get(&mask, ((size_t)range + 63) / 64 * 8) != hipSuccess)
        split = false;
    {
        if (split) {
            if (simple)
                hipLaunchKernelGGL(k_dedup_mask<true>, dim3(mat_blocks),
                                   dim3(512), 0, 0, dc, *qk, row_begin,
                                   row_end, mask);
            else
                hipLaunchKernelGGL(k_dedup_mask<false>, dim3(mat_blocks),
                                   dim3(512), 0, 0, dc, *q, row_begin,
                                   row_end, mask);
        }
        #define MAT_LAUNCH(S, K, R, M, SPm)                                  \
            hipLaunchKernelGGL((k_dedup_mat<S, K, R, M, SPm>),               \
                               dim3(mat_blocks),                             \
                               dim3(512), 0, 0, dc, *qk, row_begin, row_end, \
                               bits_total, sppad, lay, (K*)keys, rids, rec,  \
                               ctr, mask)
        #define MAT_PICK(S, K, R) \
            do { if (split) { if (sppad.n) MAT_LAUNCH(S, K, R, true, true);  \
                              else MAT_LAUNCH(S, K, R, true, false); }       \
                 else { if (sppad.n) MAT_LAUNCH(S, K, R, false, true);       \
                        else MAT_LAUNCH(S, K, R, false, false); } } while (0)
        /* vector-load mat: all padded conjunct columns 4-byte physical
         * (u32 narrow / string dict), SIMPLE spec-pack, rowid mode.
         * BK_MAT_VEC=0 falls back to the strided kernel. */
        /* default ON (parity-validated vs the strided mat + full GPU suite;
         * -31% mat at 1e7-1e8 rows, a wash at 1e9); BK_MAT_VEC: 0 = off,
         * 1 = conditional key pack, 2 = unconditional vector key pack */
        int vec_mode = 1;
        if (const char* e = getenv("BK_MAT_VEC")) vec_mode = atoi(e);
        bool vec = simple && !recmode && !split && sppad.n != 0 &&
                   vec_mode != 0;
        auto vec4 = [&](int col) {
            const DevCol& vc = dc.c[col];
            /* physical width <= 4 and a pure width mask (u8/u16/u32
             * narrow; wide string dicts are lshift 2 mask 2^32-1) */
            return vc.lshift <= 2 &&
                   vc.mask == (0xFFFFFFFFull >> (32 - (8u << vc.lshift)));
        };
        if (vec)
            for (int k = 0; k < 4; k++)
                if (!vec4(qpad.conjuncts[k].col)) vec = false;
        bool ukey = vec && vec_mode == 2 && vec4(qpad.group_cols[0]) &&
                    vec4(qpad.group_cols[1]);
        if (vec) {
            /* the vec mat prefers a near-flat grid (few grid-stride
             * iterations): 32768 blocks measured -1% vs 8192 at 1e9 rows
             * (tools/sweep_matblocks.py), clamped so small ranges don't
             * launch empty blocks (512 lanes x 16 rows per block per
             * iteration); BK_MAT_BLOCKS still overrides */
            int vblocks = getenv("BK_MAT_BLOCKS")
                ? mat_blocks
                : (int)std::min<int64_t>(32768, (range + 8191) / 8192);
            #define MATV_LAUNCH(K, U)                                        \
                hipLaunchKernelGGL((k_dedup_mat_vec<K, U>),                  \
                                   dim3(vblocks), dim3(512), 0, 0, dc,       \
                                   qpad, row_begin, row_end, bits_total,     \
                                   sppad, (K*)keys, rids, ctr)
            if (key32) { if (ukey) MATV_LAUNCH(uint32_t, true);
                         else MATV_LAUNCH(uint32_t, false); }
            else       { if (ukey) MATV_LAUNCH(uint64_t, true);
                         else MATV_LAUNCH(uint64_t, false); }
            #undef MATV_LAUNCH
        } else if (simple) {
            if (key32) { if (recmode) MAT_PICK(true, uint32_t, true);
                         else MAT_PICK(true, uint32_t, false); }
            else       { if (recmode) MAT_PICK(true, uint64_t, true);
                         else MAT_PICK(true, uint64_t, false); }
        } else {
            if (key32) { if (recmode) MAT_PICK(false, uint32_t, true);
                         else MAT_PICK(false, uint32_t, false); }
            else       { if (recmode) MAT_PICK(false, uint64_t, true);
                         else MAT_PICK(false, uint64_t, false); }
        }
        #undef MAT_PICK
        #undef MAT_LAUNCH
    }
    BK_TRY("sorted", hipGetLastError(), nullptr);
    uint64_t n = 0;
    BK_TRY("sorted", hipMemcpy(&n, ctr, 8, hipMemcpyDeviceToHost), nullptr);
    tm.record();

    uint64_t ngroups = 0;
    if (n > 0) {
        BK_TRY("sorted", bufs.get(&keys2, (size_t)n * ksz), nullptr);
        BK_TRY("sorted", bufs.get(&rids2, (size_t)n * 4), nullptr);
        if (recmode)   /* sort values = record indices */
            dev_iota(rids, n, 2048);
        const unsigned end_bit = (unsigned)(bits_total + 8);
        if (key32)
            BK_TRY("sorted", dev_sort_pairs(bufs, (uint32_t*)keys, (uint32_t*)keys2,
                                            rids, rids2, (size_t)n, 0, end_bit),
                   nullptr);
        else
            BK_TRY("sorted", dev_sort_pairs(bufs, (uint64_t*)keys, (uint64_t*)keys2,
                                            rids, rids2, (size_t)n, 0, end_bit),
                   nullptr);
        tm.record();
        BK_TRY("sorted", bufs.get(&f, (size_t)n * 4), nullptr);
        BK_TRY("sorted", bufs.get(&gidx, (size_t)n * 4), nullptr);
        if (key32)
            hipLaunchKernelGGL(k_dedup_heads<uint32_t>, dim3(2048), dim3(256),
                               0, 0, (const uint32_t*)keys2, n, f);
        else
            hipLaunchKernelGGL(k_dedup_heads<uint64_t>, dim3(2048), dim3(256),
                               0, 0, (const uint64_t*)keys2, n, f);
        BK_TRY("sorted", dev_inclusive_scan(bufs, f, gidx, (size_t)n,
                                            DevPlus<uint32_t>()), nullptr);
        uint32_t ng32 = 0;
        BK_TRY("sorted", hipMemcpy(&ng32, gidx + (n - 1), 4, hipMemcpyDeviceToHost),
               nullptr);
        ngroups = ng32;
    } else {
        tm.record();
    }
    tm.record();

    BkgAggOut* o = new BkgAggOut();
    o->q = *q;
    if (agg_alloc(o, std::max<int64_t>(1, (int64_t)ngroups)) != 0) {
        bkgpu_agg_free(o); return nullptr;
    }
    /* dense table: fill = ngroups (merge's capacity check then always
     * rebuilds to a hash table first), rows_passed = survivors */
    BK_TRY("sorted", hipMemcpy(o->ctrs, &ngroups, 8, hipMemcpyHostToDevice),
           (bkgpu_agg_free(o), nullptr));
    BK_TRY("sorted", hipMemcpy(o->ctrs + 1, &n, 8, hipMemcpyHostToDevice),
           (bkgpu_agg_free(o), nullptr));
    if (n > 0) {
        #define EMIT_LAUNCH(NAv, K, R)                                       \
            hipLaunchKernelGGL((k_dedup_emit<NAv, K, R>), dim3(4096),        \
                               dim3(256), 0, 0, dc, *q, row_begin,           \
                               bits_total, sp, lay, (const K*)keys2, rids2,  \
                               rec, gidx, n, o->table)
        bool na4 = q->n_aggs <= 4;
        if (key32) {
            if (recmode) { if (na4) EMIT_LAUNCH(4, uint32_t, true);
                           else EMIT_LAUNCH(8, uint32_t, true); }
            else         { if (na4) EMIT_LAUNCH(4, uint32_t, false);
                           else EMIT_LAUNCH(8, uint32_t, false); }
        } else {
            if (recmode) { if (na4) EMIT_LAUNCH(4, uint64_t, true);
                           else EMIT_LAUNCH(8, uint64_t, true); }
            else         { if (na4) EMIT_LAUNCH(4, uint64_t, false);
                           else EMIT_LAUNCH(8, uint64_t, false); }
        }
        #undef EMIT_LAUNCH
        BK_TRY("sorted", hipGetLastError(), (bkgpu_agg_free(o), nullptr));
    }
    tm.record();
    tm.finish(o, NAMESD);
    o->dirty = true;
    o->rows_passed = (int64_t)n;   /* compaction stays lazy (see filter_agg) */
    return o;
}
