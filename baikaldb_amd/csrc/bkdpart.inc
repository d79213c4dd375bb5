/* ------------------------------------------------------------------ */
/* DENSE-SPAN partition pipeline ("dpart")                             */
/*                                                                     */
/* When the packed group-key domain is small — the product of the      */
/* per-key encoding spans fits ~2^23 dense ids — the hash-partitioned  */
/* aggregate (k_part_histo/scatter/agg, hash buckets + LDS claim       */
/* chains) is replaced by a RANGE partition on the dense key id:       */
/*                                                                     */
/*   did = (enc(k0) - min0) << k1bits | (enc(k1) - min1)               */
/*   bucket = did >> shift        (2^shift dense ids per bucket)       */
/*                                                                     */
/* so pass 3 aggregates each bucket into a DIRECT-INDEXED LDS array    */
/* (ds-atomics at lidx = did - bucket_base): no hashing, no probe or   */
/* claim chains, no generation flushes — the levers DESIGN.md §6 names */
/* as the k_part_agg latency bound. The global result is a dense array */
/* too (per-slot {touched, value words}): k_dcompact turns it straight */
/* into the wire blob, and dense_to_hash rebuilds a hash table from    */
/* that blob only when merge / rollup need one.                        */
/*                                                                     */
/* Semantics identical to the hash path (same per-agg atomic op set,   */
/* agg_node.cpp:405-587 / agg_fn_call.cpp:496-830): COUNT/SUM int64    */
/* bit-exact (wrapping adds), SUM/AVG double within the stated         */
/* tolerance (order-free f64 atomics), MIN/MAX exact on the order-     */
/* preserving encoding. Eligibility (dense_spans):    1-2 fn-free      */
/* non-nullable group keys, no declared group_bits, non-nullable       */
/* aggregate inputs (per-agg non-null counts == per-group row count,   */
/* synthesized from one `touched` counter — 4x fewer atomics).         */
/*                                                                     */
/* Records are 4-byte-granular: [did u32][narrow u32 deltas][wide u64] */
/* — an INT64 aggregate input whose value span fits 32 bits travels as */
/* a u32 delta (stats-driven), so the config-3 record is 24 B against  */
/* the hash path's 32 B (scatter write + agg read traffic).            */
/* ------------------------------------------------------------------ */

#define DPART_T 16            /* rows per lane per tile (16 B vec loads) */

struct DenseSpec {
    uint64_t base0, base1;       /* encoded minima of group keys 0 / 1 */
    uint32_t k1bits;             /* log2 dense slots for key 1 (0: 1 key) */
    uint32_t span;               /* total dense ids = (span0+1) << k1bits */
    uint32_t shift;              /* log2 dense ids per bucket */
    uint32_t P;                  /* ceil(span / 2^shift) buckets */
    uint32_t hshift;             /* shift-k1bits when >=0: bucket from k0
                                    alone (histo skips the k1 column);
                                    0xFFFFFFFF otherwise */
    int32_t  nv;                 /* value words per dense slot */
    int32_t  vslot[BK_MAX_AGGS]; /* dense value index per agg; -1 none */
    int32_t  vop[BK_MAX_AGGS];   /* per VALUE SLOT: 0 add-u64, 1 add-f64,
                                    2 max-u64 (flush op) */
};

struct DRecLayout {
    int32_t  nwords;               /* u64 words per record; word0.lo = did */
    int32_t  off32[BK_MAX_AGGS];   /* u32 offset of agg field; -1 none */
    int32_t  wide[BK_MAX_AGGS];    /* 1 = 8-byte field (off32 even) */
    uint64_t vbase[BK_MAX_AGGS];   /* narrow fields: value = vbase + delta
                                      (i64 domain for SUM, enc for MIN/MAX) */
    /* PACK32 split records (eager scatter only): when did's bits plus every
     * narrow field's stats-derived bits fit one u32, the record splits into
     * a u32 hdr stream (did << pkdidsh | fields) and an aligned stream of
     * the wide u64 payload words — the config3-class record drops 24->20 B
     * on both the scatter write and the dagg read, and every store/load is
     * naturally aligned. */
    int32_t  pk;                   /* 1 = split layout active */
    int32_t  pknf;                 /* wide payload words per record */
    uint32_t pkdidsh;              /* did shift in hdr = total narrow bits */
    uint32_t pksh[2];              /* per-narrow-field shift in hdr */
    uint32_t pkmask[2];            /* per-narrow-field mask */
};

struct DDesc { uint32_t bucket; uint32_t cnt; uint64_t start; };

/* dense id of row r (keys verified non-null by dense_spans) */
template <bool SIMPLE>
__device__ __forceinline__ uint32_t dense_did(const DevCols& cols,
                                              const BkQuerySpec& q,
                                              const DenseSpec& ds, int64_t r) {
    const DevCol& c0 = cols.c[q.group_cols[0]];
    uint64_t d0 = (SIMPLE ? enc_value_nf(c0, r) : enc_value(c0, r)) - ds.base0;
    if (ds.k1bits == 0) return (uint32_t)d0;
    const DevCol& c1 = cols.c[q.group_cols[1]];
    uint64_t d1 = (SIMPLE ? enc_value_nf(c1, r) : enc_value(c1, r)) - ds.base1;
    return (uint32_t)((d0 << ds.k1bits) | d1);
}

/* ---- whole-tile column staging ----
 * PMC measured the per-4-row 16 B sub-chunk loads re-fetching each 64 B
 * line up to ~4x from HBM (42 GB read on an 11 GB-algorithmic histo): at 8
 * waves/CU the L1 evicts a line between one lane's sub-chunk touches. The
 * stagers below read a column's WHOLE 16- or 8-row tile with back-to-back
 * loads (one L1-resident line walk), branched on the launch-uniform
 * physical width so every extraction index is compile-time (no scratch).
 * Values return in by-value structs — array parameters decay to pointers
 * and spill. */
struct Enc16 { uint32_t d[16]; };
struct Enc8 { uint32_t d[8]; };
struct W8 { uint64_t v[8]; };

/* ((base + raw) ^ flip) - sub for 16 consecutive rows of a width<=4 column
 * (u32 result: dense ids and narrow record fields are < 2^32 by plan) */
__device__ __forceinline__ Enc16 stage_enc16(const DevCol& c, int64_t rb,
                                             uint64_t flip, uint64_t sub) {
    Enc16 o;
    const char* p = (const char*)c.data + (rb << c.lshift);
    if (c.lshift == 2) {
        uint64_t w[8];
        #pragma unroll
        for (int i = 0; i < 4; i++)
            __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            uint64_t raw = (w[j >> 1] >> ((j & 1) * 32)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    } else if (c.lshift == 1) {
        uint64_t w[4];
        #pragma unroll
        for (int i = 0; i < 2; i++)
            __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            uint64_t raw = (w[j >> 2] >> ((j & 3) * 16)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    } else {
        uint64_t w[2];
        __builtin_memcpy(w, p, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            uint64_t raw = (w[j >> 3] >> ((j & 7) * 8)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    }
    return o;
}

/* 8 consecutive rows from row rs + vo: rs is the wave's (scalar) base row, vo
 * the lane's small offset, kept apart so the address is a scalar base plus a
 * 32-bit lane offset instead of a 64-bit value per lane */
__device__ __forceinline__ Enc8 stage_enc8(const DevCol& c, int64_t rs,
                                           uint32_t vo, uint64_t flip,
                                           uint64_t sub) {
    Enc8 o;
    const char* p = (const char*)c.data + (rs << c.lshift)
                    + (size_t)(vo << c.lshift);
    if (c.lshift == 2) {
        uint64_t w[4];
        #pragma unroll
        for (int i = 0; i < 2; i++)
            __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t raw = (w[j >> 1] >> ((j & 1) * 32)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    } else if (c.lshift == 1) {
        uint64_t w[2];
        __builtin_memcpy(w, p, 16);
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t raw = (w[j >> 2] >> ((j & 3) * 16)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    } else {
        uint64_t w;
        __builtin_memcpy(&w, p, 8);
        #pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t raw = (w >> (j * 8)) & c.mask;
            o.d[j] = (uint32_t)((((uint64_t)c.base + raw) ^ flip) - sub);
        }
    }
    return o;
}

/* 8 consecutive rows of a width-8 column (f64 bits / wide int64): one full
 * 64 B line, 4 back-to-back 16 B loads */
__device__ __forceinline__ W8 stage_w8(const void* data, int64_t rs,
                                       uint32_t vo) {
    W8 o;
    const char* p = (const char*)data + ((uint64_t)rs << 3) + (size_t)(vo << 3);
    #pragma unroll
    for (int i = 0; i < 4; i++)
        __builtin_memcpy(&o.v[2 * i], p + 16 * i, 16);
    return o;
}

/* 16-row compare mask of one conjunct (width-branched staged loads) */
__device__ __forceinline__ uint32_t conj_mask16(const BkConjunct& cj,
                                                const DevCol& c, int64_t rb) {
    /* reuse the enc stager with flip=0, sub=0: d[j] = base + raw = value.
     * Conjunct values fit 32 bits only if the column is narrow-stored with
     * base 0 — NOT guaranteed (frame-of-reference base). Compare in 64-bit
     * against lit - base instead: raw & mask is < 2^32, lit' = lit - base
     * may be any int64 -> do the compare on (int64)(base + raw). */
    const char* p = (const char*)c.data + (rb << c.lshift);
    uint32_t m = 0;
    const int64_t lit = cj.lit_i;
    const int op3 = 3 * cj.op;
    if (c.lshift == 2) {
        uint64_t w[8];
        #pragma unroll
        for (int i = 0; i < 4; i++)
            __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            int64_t v = (int64_t)((uint64_t)c.base
                                  + ((w[j >> 1] >> ((j & 1) * 32)) & c.mask));
            int cmp = (v > lit) - (v < lit);
            m |= ((0x19D2Au >> (op3 + cmp + 1)) & 1u) << j;
        }
    } else if (c.lshift == 1) {
        uint64_t w[4];
        #pragma unroll
        for (int i = 0; i < 2; i++)
            __builtin_memcpy(&w[2 * i], p + 16 * i, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            int64_t v = (int64_t)((uint64_t)c.base
                                  + ((w[j >> 2] >> ((j & 3) * 16)) & c.mask));
            int cmp = (v > lit) - (v < lit);
            m |= ((0x19D2Au >> (op3 + cmp + 1)) & 1u) << j;
        }
    } else {
        uint64_t w[2];
        __builtin_memcpy(w, p, 16);
        #pragma unroll
        for (int j = 0; j < 16; j++) {
            int64_t v = (int64_t)((uint64_t)c.base
                                  + ((w[j >> 3] >> ((j & 7) * 8)) & c.mask));
            int cmp = (v > lit) - (v < lit);
            m |= ((0x19D2Au >> (op3 + cmp + 1)) & 1u) << j;
        }
    }
    return m;
}

/* pass 1: predicate -> per-lane 16-row passbits word (u16) + per-block
 * bucket histogram. VEC: the conjunct columns (padded to 4, physical width
 * <= 4 B) read with one unconditional 16 B load per 4-row sub-chunk — the
 * k_dedup_mat_vec load shape (bkdedup.inc), which removes the per-load
 * s_waitcnt serialization the strided histo pays. KV: the bucket key
 * column(s) are ALSO read with unconditional 16 B vector loads and the
 * bucket computed branchlessly per row (KV=1: bucket from key 0 alone,
 * ds.hshift; KV=2: both keys) — the masked per-row key gather (KV=0)
 * serializes a ~16-deep dependent load+atomic chain per lane and measured
 * 0.6-1.2 TB/s where the streaming ceiling is ~3. */
template <int BS, bool SIMPLE, bool VEC, int KV, int NCJ = 4>
__global__ void __launch_bounds__(BS)
k_dhisto(DevCols cols, BkQuerySpec q, DenseSpec ds, int64_t row_begin,
         int64_t row_end, uint16_t* passbits, uint32_t* H, uint32_t* totals,
         uint64_t* rows_passed) {
    constexpr int T = DPART_T;
    extern __shared__ __attribute__((aligned(16))) uint64_t laux_[];
    uint32_t* lhist = (uint32_t*)(laux_ + 1);
    if (threadIdx.x == 0) laux_[0] = 0;
    for (uint32_t b = threadIdx.x; b < ds.P; b += BS) lhist[b] = 0;
    __syncthreads();
    int64_t gstride = (int64_t)gridDim.x * BS;
    int64_t lin = (int64_t)blockIdx.x * BS + threadIdx.x;
    int64_t my_passed = 0;
    for (int64_t b0 = row_begin + lin * T; b0 < row_end; b0 += gstride * T) {
        uint32_t pb = 0;
        if (VEC && b0 + T <= row_end) {
            pb = 0xFFFFu;
            #pragma unroll
            for (int k = 0; k < NCJ; k++) {
                if (!pb) break;   /* whole tile failed: skip further loads */
                pb &= conj_mask16(q.conjuncts[k],
                                  cols.c[q.conjuncts[k].col], b0);
            }
            if (KV >= 1 && pb) {   /* key loads skipped for dead tiles */
                const DevCol& c0 = cols.c[q.group_cols[0]];
                uint64_t flip0 = c0.type == BK_STRING ? 0 : (1ull << 63);
                Enc16 dd = stage_enc16(c0, b0, flip0, ds.base0);
                uint32_t sh = ds.hshift;
                if (KV == 2) {
                    const DevCol& c1 = cols.c[q.group_cols[1]];
                    uint64_t flip1 = c1.type == BK_STRING ? 0 : (1ull << 63);
                    Enc16 d1 = stage_enc16(c1, b0, flip1, ds.base1);
                    #pragma unroll
                    for (int j = 0; j < 16; j++)
                        dd.d[j] = (dd.d[j] << ds.k1bits) | d1.d[j];
                    sh = ds.shift;
                }
                #pragma unroll
                for (int j = 0; j < 16; j++)
                    if ((pb >> j) & 1u) atomicAdd(&lhist[dd.d[j] >> sh], 1u);
            }
        } else {
            #pragma unroll
            for (int j = 0; j < T; j++) {
                int64_t r = b0 + j;
                if (r < row_end && row_passes<SIMPLE>(cols, q, r))
                    pb |= 1u << j;
            }
        }
        passbits[(b0 - row_begin) / T] = (uint16_t)pb;
        my_passed += __popc(pb);
        if (KV == 0 || !(VEC && b0 + T <= row_end)) {
            /* masked per-row bucket (generic shapes and tail tiles) */
            uint32_t m = pb;
            while (m) {
                int j = __builtin_ctz(m);
                m &= m - 1;
                int64_t r = b0 + j;
                uint32_t b;
                if (ds.hshift != 0xFFFFFFFFu) {
                    const DevCol& c0 = cols.c[q.group_cols[0]];
                    uint64_t d0 = (SIMPLE ? enc_value_nf(c0, r)
                                          : enc_value(c0, r)) - ds.base0;
                    b = (uint32_t)(d0 >> ds.hshift);
                } else {
                    b = dense_did<SIMPLE>(cols, q, ds, r) >> ds.shift;
                }
                atomicAdd(&lhist[b], 1u);
            }
        }
    }
    long long wsum = my_passed;
    for (int off = 32; off > 0; off >>= 1) wsum += __shfl_down(wsum, off, 64);
    if ((threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)&laux_[0], (unsigned long long)wsum);
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd((unsigned long long*)rows_passed,
                  (unsigned long long)laux_[0]);
    /* per-block counts for the scatter's reservation, bucket totals for the
     * scan (as k_part_histo) */
    for (uint32_t b = threadIdx.x; b < ds.P; b += BS) {
        uint32_t n = lhist[b];
        H[(size_t)blockIdx.x * ds.P + b] = n;
        if (n) atomicAdd(&totals[b], n);
    }
}

/* place one 32- or 64-bit field into the record register block */
__device__ __forceinline__ void drec_put(uint64_t* regs, int off32, int wide,
                                         uint64_t v) {
    if (wide) {
        regs[off32 >> 1] = v;
    } else if (off32 & 1) {
        regs[off32 >> 1] |= v << 32;
    } else {
        regs[off32 >> 1] |= v & 0xFFFFFFFFull;
    }
}
__device__ __forceinline__ uint64_t drec_get(const uint64_t* my, int off32,
                                             int wide) {
    uint64_t w = my[off32 >> 1];
    if (wide) return w;
    return (off32 & 1) ? (w >> 32) : (w & 0xFFFFFFFFull);
}

/* scalar masked single-row record build (k_dscatter only — the eager
 * kernel's tail builds records with compile-time offsets instead: a
 * noinline call here was measured to cost the EAGER kernel 2.6 KB/lane of
 * scratch ALLOCATION, which throttles resident waves even when the tail
 * path never executes). */
template <bool SIMPLE>
__device__ __forceinline__ void dscatter_row(
        const DevCols& cols, const BkQuerySpec& q, const DenseSpec& ds,
        const DRecLayout& lay, int64_t r, uint32_t* lcur, uint64_t* rec) {
    uint32_t did = dense_did<SIMPLE>(cols, q, ds, r);
    uint64_t regs[8];
    #pragma unroll
    for (int w = 0; w < 8; w++) regs[w] = 0;
    regs[0] = did;
    for (int32_t a = 0; a < q.n_aggs; a++) {
        if (lay.off32[a] < 0) continue;
        const BkAggSpec& as = q.aggs[a];
        AggIn v = agg_input(cols, q, as, q.agg_in_types[a], r);
        uint64_t f = 0;
        switch (as.agg_type) {
            case BK_AGG_SUM:
                if (q.agg_in_types[a] == BK_DOUBLE) memcpy(&f, &v.d, 8);
                else f = (uint64_t)v.i - (lay.wide[a] ? 0 : lay.vbase[a]);
                break;
            case BK_AGG_AVG:
                memcpy(&f, &v.d, 8);
                break;
            case BK_AGG_MIN:
            case BK_AGG_MAX:
                f = agg_enc(cols, as, q.agg_in_types[a], v, r)
                    - (lay.wide[a] ? 0 : lay.vbase[a]);
                break;
            default: break;
        }
        drec_put(regs, lay.off32[a], lay.wide[a], f);
    }
    uint32_t b = did >> ds.shift;
    uint32_t pos = atomicAdd(&lcur[b], 1u);
    scatter_store_rec(rec + (size_t)pos * lay.nwords, regs, lay.nwords);
}

/* pass 2: scatter dense records into bucket-contiguous regions. MUST share
 * k_dhisto's grid/block AND row->tile mapping (H rows are per-block). */
template <int BS, bool SIMPLE>
__global__ void __launch_bounds__(BS)
k_dscatter(DevCols cols, BkQuerySpec q, DenseSpec ds, DRecLayout lay,
           int64_t row_begin, int64_t row_end, const uint16_t* passbits,
           const uint32_t* H, uint32_t* base, uint64_t* rec) {
    constexpr int T = DPART_T;
    extern __shared__ __attribute__((aligned(16))) uint64_t lmem[];
    uint32_t* lcur = (uint32_t*)lmem;
    for (uint32_t b = threadIdx.x; b < ds.P; b += BS)
        lcur[b] = part_reserve(H, base, ds.P, b);
    __syncthreads();
    int64_t gstride = (int64_t)gridDim.x * BS;
    int64_t lin = (int64_t)blockIdx.x * BS + threadIdx.x;
    for (int64_t b0 = row_begin + lin * T; b0 < row_end; b0 += gstride * T) {
        uint32_t m = passbits[(b0 - row_begin) / T];
        while (m) {
            int j = __builtin_ctz(m);
            m &= m - 1;
            dscatter_row<SIMPLE>(cols, q, ds, lay, b0 + j, lcur, rec);
        }
    }
}

/* one field's LDS update (shared by the AoS and PACK32 record readers) */
__device__ __forceinline__ void dagg_apply(const BkQuerySpec& q,
                                           const DRecLayout& lay, int32_t a,
                                           uint64_t f, uint64_t* lv) {
    switch (q.aggs[a].agg_type) {
        case BK_AGG_SUM:
            if (q.agg_in_types[a] == BK_DOUBLE) {
                double dd;
                memcpy(&dd, &f, 8);
                atomic_add_f64_lds(lv, dd);
            } else {
                uint64_t v = lay.wide[a] ? f : lay.vbase[a] + f;
                atomicAdd((unsigned long long*)lv, (unsigned long long)v);
            }
            break;
        case BK_AGG_AVG: {
            double dd;
            memcpy(&dd, &f, 8);
            atomic_add_f64_lds(lv, dd);
            break;
        }
        case BK_AGG_MIN: {
            uint64_t e = lay.wide[a] ? f : lay.vbase[a] + f;
            atomicMax((unsigned long long*)lv, (unsigned long long)~e);
            break;
        }
        case BK_AGG_MAX: {
            uint64_t e = lay.wide[a] ? f : lay.vbase[a] + f;
            atomicMax((unsigned long long*)lv, (unsigned long long)e);
            break;
        }
        default: break;
    }
}

/* one record's LDS updates (k_dagg's ILP legs AND the hot-bucket absorb
 * path inside the ABS eager scatter — definition above k_dscatter_e) */
__device__ __forceinline__ void dagg_rec(const BkQuerySpec& q,
                                         const DenseSpec& ds,
                                         const DRecLayout& lay,
                                         const uint64_t* my, uint32_t dbase,
                                         uint64_t* lval, uint32_t* ltou,
                                         int nv) {
    uint32_t l = (uint32_t)my[0] - dbase;
    atomicAdd(&ltou[l], 1u);
    for (int32_t a = 0; a < q.n_aggs; a++) {
        if (lay.off32[a] < 0) continue;
        uint64_t f = drec_get(my, lay.off32[a], lay.wide[a]);
        dagg_apply(q, lay, a, f, &lval[(size_t)l * nv + ds.vslot[a]]);
    }
}

/* PACK32 record: narrow fields extract from the u32 hdr by launch-uniform
 * shift/mask (register ops, no runtime-indexed array — scratch-safe); wide
 * fields load from the payload stream in field order. */
__device__ __forceinline__ void dagg_rec_pk(const BkQuerySpec& q,
                                            const DenseSpec& ds,
                                            const DRecLayout& lay,
                                            uint32_t hw, const uint64_t* pay,
                                            uint32_t dbase, uint64_t* lval,
                                            uint32_t* ltou, int nv) {
    uint32_t l = (hw >> lay.pkdidsh) - dbase;
    atomicAdd(&ltou[l], 1u);
    int wi = 0;
    for (int32_t a = 0; a < q.n_aggs; a++) {
        if (lay.off32[a] < 0) continue;
        uint64_t f;
        if (!lay.wide[a]) {
            int s = lay.off32[a] - 1;          /* canonical order: slot 1,2 */
            f = (hw >> lay.pksh[s]) & lay.pkmask[s];
        } else {
            f = pay[wi++];
        }
        dagg_apply(q, lay, a, f, &lval[(size_t)l * nv + ds.vslot[a]]);
    }
}

/* EAGER scatter: the canonical dense record layout
 *   [did u32][NAR narrow u32 fields][pad][NF wide u64 fields]
 * compiled out per (NK keys, NAR, NF) shape. Every source column is read
 * with unconditional 16 B vector loads per 4-row sub-chunk (wide columns:
 * 2x16 B), so the gather never serializes on the pass branch; sub-chunks
 * with no surviving rows skip their loads entirely (selectivity-adaptive).
 * Tail tiles take the masked scalar path (same records via DRecLayout). */
struct DScatE {
    int32_t  ncol[2];    /* narrow agg field source columns */
    uint64_t nflip[2];   /* xor before base-subtract (enc for MIN/MAX) */
    uint64_t nsub[2];    /* field = ((base+raw)^nflip) - nsub */
    int32_t  wcol[3];    /* wide field source columns (phys width 8) */
    int32_t  wmode[3];   /* 0 raw, 1 xor 2^63 (MIN/MAX i64), 2 f64-enc */
    /* ABS absorb plan (all launch-uniform; compile-time NAR/NF shape):
     * value slot index + op per field. nop: 0 add, 1 max (MAX), 2 max of
     * ~v (MIN). wop: 0 f64 add, 1 u64 add, 2 max, 3 max of ~v. The
     * absorbed update is exactly dagg_rec's per-record arithmetic with the
     * field selection resolved at compile time (the runtime agg loop there
     * measured ~+40% on the scatter under 39% absorption divergence). */
    int32_t  naslot[2];
    int32_t  nop[2];
    int32_t  waslot[3];
    int32_t  wop[3];
};

/* ABS: hot-bucket absorption. The host knows the exact per-bucket survivor
 * histogram (h_tot, synced before the scatter launches); when one bucket
 * holds a large fraction of the survivors (skewed group keys — the
 * reference's planner faces the same Zipf reality, agg_node.cpp hash
 * tables just eat it), the ABS instantiation aggregates that bucket's rows
 * DIRECTLY into an LDS dense array (same ds-atomic ops as k_dagg) instead
 * of writing records: the whole scatter-write + dagg-read round trip is
 * skipped for the hottest bucket. Each block streams its LDS array to a
 * per-block slab at the end (coalesced, no atomics); k_dabs_reduce folds
 * the slabs into gvals/gtouch (column-major over blocks: fully coalesced,
 * one atomic per live slot). Selection is per chunk from measured counts —
 * no stats, no priors; flat data never qualifies (host gate BK_DABS_MIN). */
template <int BS, int NK, int NAR, int NF, bool ABS = false, bool PK = false>
__global__ void __launch_bounds__(BS)
k_dscatter_e(DevCols cols, BkQuerySpec q, DenseSpec ds, DRecLayout lay,
             DScatE prm, int64_t row_begin, int64_t row_end,
             const uint16_t* passbits, const uint32_t* H, uint32_t* base,
             uint64_t* rec, uint32_t* hdr, uint32_t hb, uint64_t* vslab, uint32_t* tslab) {
    constexpr int T = DPART_T;
    constexpr int NU32 = 1 + NAR;
    constexpr int WOFF = (NU32 + 1) / 2;          /* wide fields word base */
    constexpr int NWORDS = NF > 0 ? WOFF + NF : (NU32 + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) uint64_t lmem[];
    const uint32_t win = ABS ? 1u << ds.shift : 0;
    const int nv = ds.nv;
    uint64_t* lval = lmem;                         /* ABS: win*nv u64 */
    uint32_t* ltou = (uint32_t*)(lmem + (ABS ? (size_t)win * nv : 0));
    uint32_t* lcur = ABS ? ltou + win : (uint32_t*)lmem;
    if (ABS) {
        for (uint32_t i = threadIdx.x; i < win * (uint32_t)nv; i += BS)
            lval[i] = 0;
        for (uint32_t i = threadIdx.x; i < win; i += BS) ltou[i] = 0;
    }
    for (uint32_t b = threadIdx.x; b < ds.P; b += BS)
        lcur[b] = part_reserve(H, base, ds.P, b);
    __syncthreads();
    int64_t gstride = (int64_t)gridDim.x * BS;
    /* the loop walks the WAVE's base row (scalar: readfirstlane of a value
     * every lane of a wave shares); a lane's rows are that base plus a small
     * lane offset. A wave's 64 tiles are 1024 consecutive rows = 128
     * half-tiles, and H counts per block, so the wave may deal them to its
     * lanes freely. When the whole span is in range, lane l takes half-tile
     * 64h + l in pass h, so neighbouring lanes stage neighbouring 8-row
     * pieces: the two halves of a 128 B line of an 8-byte column load in the
     * same instructions, not a j-loop apart (4-byte columns share a line over
     * 4 lanes, 2-byte columns coalesce fully). passbits is little-endian u16
     * per tile: byte k = half-tile k. A wave that crosses row_end keeps
     * tile-per-lane, scalar tail tile included. */
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t wlin = (int64_t)blockIdx.x * BS +
        (__builtin_amdgcn_readfirstlane((int)threadIdx.x) & ~63);
    for (int64_t wb = row_begin + wlin * T; wb < row_end; wb += gstride * T) {
        const bool whole = wb + 64 * T <= row_end;
        uint32_t pb;
        if (whole) {
            const uint8_t* pby =
                (const uint8_t*)passbits + (wb - row_begin) / 8;
            pb = (uint32_t)pby[lane] | ((uint32_t)pby[64 + lane] << 8);
        } else {
            if (wb + lane * T >= row_end) continue;
            pb = passbits[(wb - row_begin) / T + lane];
        }
        if (!pb) continue;
        if (!whole && wb + lane * T + T > row_end) {   /* tail tile: scalar,
                                                      same compile-time
                                                      field walk */
            const int64_t b0 = wb + lane * T;
            while (pb) {
                int j = __builtin_ctz(pb);
                pb &= pb - 1;
                int64_t r = b0 + j;
                const DevCol& c0 = cols.c[q.group_cols[0]];
                uint64_t flip0 = c0.type == BK_STRING ? 0 : (1ull << 63);
                uint64_t d0 = (((uint64_t)cell_i64(c0, r)) ^ flip0)
                              - ds.base0;
                uint32_t did;
                if (NK == 1) {
                    did = (uint32_t)d0;
                } else {
                    const DevCol& c1 = cols.c[q.group_cols[1]];
                    uint64_t flip1 = c1.type == BK_STRING ? 0 : (1ull << 63);
                    uint64_t d1 = (((uint64_t)cell_i64(c1, r)) ^ flip1)
                                  - ds.base1;
                    did = (uint32_t)((d0 << ds.k1bits) | d1);
                }
                uint64_t regs[NWORDS];
                #pragma unroll
                for (int w = 0; w < NWORDS; w++) regs[w] = 0;
                regs[0] = did;
                #pragma unroll
                for (int i = 0; i < NAR; i++) {
                    const DevCol& c = cols.c[prm.ncol[i]];
                    uint64_t f = (((uint64_t)cell_i64(c, r)) ^ prm.nflip[i])
                                 - prm.nsub[i];
                    if ((1 + i) & 1) regs[(1 + i) >> 1] |= f << 32;
                    else             regs[(1 + i) >> 1] |= f & 0xFFFFFFFFull;
                }
                #pragma unroll
                for (int i = 0; i < NF; i++) {
                    uint64_t raw =
                        ((const uint64_t*)cols.c[prm.wcol[i]].data)[r];
                    uint64_t v = raw;
                    if (prm.wmode[i] == 1) v = raw ^ (1ull << 63);
                    else if (prm.wmode[i] == 2)
                        v = raw ^ ((uint64_t)((int64_t)raw >> 63)
                                   | 0x8000000000000000ull);
                    else if (prm.wmode[i] == 3) {
                        double dc = (double)(int64_t)raw;
                        memcpy(&v, &dc, 8);
                    }
                    regs[WOFF + i] = v;
                }
                if (ABS && did - hb < win) {
                    dagg_rec(q, ds, lay, regs, hb, lval, ltou, nv);
                    continue;
                }
                uint32_t b = did >> ds.shift;
                uint32_t pos = atomicAdd(&lcur[b], 1u);
                if (PK) {
                    uint32_t hw = did << lay.pkdidsh;
                    #pragma unroll
                    for (int i = 0; i < NAR; i++) {
                        uint64_t w = regs[(1 + i) >> 1];
                        uint32_t f = (uint32_t)(((1 + i) & 1) ? (w >> 32)
                                                              : w);
                        hw |= (f & lay.pkmask[i]) << lay.pksh[i];
                    }
                    hdr[pos] = hw;
                    #pragma unroll
                    for (int i = 0; i < NF; i++)
                        rec[(size_t)pos * NF + i] = regs[WOFF + i];
                } else {
                    uint64_t* dst = rec + (size_t)pos * NWORDS;
                    #pragma unroll
                    for (int w = 0; w < NWORDS; w++) dst[w] = regs[w];
                }
            }
            continue;
        }
        /* half-tile (8-row) staged processing: every source column's bytes
         * for the 8 rows load back-to-back (width-branched stagers), so a
         * 64 B line is touched in adjacent instructions instead of being
         * re-fetched per 4-row sub-chunk (PMC: 76 GB read vs ~21 GB
         * algorithmic before this restructure) */
        #pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t sub8 = (pb >> (8 * h)) & 0xFFu;
            if (!sub8) continue;                   /* no loads, no work */
            const uint32_t vo = whole ? 8 * (64 * h + lane)
                                      : T * lane + 8 * h;
            const DevCol& c0 = cols.c[q.group_cols[0]];
            uint64_t flip0 = c0.type == BK_STRING ? 0 : (1ull << 63);
            Enc8 dd = stage_enc8(c0, wb, vo, flip0, ds.base0);
            if (NK == 2) {
                const DevCol& c1 = cols.c[q.group_cols[1]];
                uint64_t flip1 = c1.type == BK_STRING ? 0 : (1ull << 63);
                Enc8 d1 = stage_enc8(c1, wb, vo, flip1, ds.base1);
                #pragma unroll
                for (int j = 0; j < 8; j++)
                    dd.d[j] = (dd.d[j] << ds.k1bits) | d1.d[j];
            }
            Enc8 nf[NAR > 0 ? NAR : 1];
            #pragma unroll
            for (int i = 0; i < NAR; i++)
                nf[i] = stage_enc8(cols.c[prm.ncol[i]], wb, vo, prm.nflip[i],
                                   prm.nsub[i]);
            W8 wf[NF > 0 ? NF : 1];
            #pragma unroll
            for (int i = 0; i < NF; i++)
                wf[i] = stage_w8(cols.c[prm.wcol[i]].data, wb, vo);
            #pragma unroll
            for (int j = 0; j < 8; j++) {
                if (!((sub8 >> j) & 1u)) continue;
                uint32_t did = dd.d[j];
                uint64_t wv[NF > 0 ? NF : 1];
                #pragma unroll
                for (int i = 0; i < NF; i++) {
                    uint64_t raw = wf[i].v[j];
                    uint64_t v = raw;
                    if (prm.wmode[i] == 1) v = raw ^ (1ull << 63);
                    else if (prm.wmode[i] == 2)
                        v = raw ^ ((uint64_t)((int64_t)raw >> 63)
                                   | 0x8000000000000000ull);
                    else if (prm.wmode[i] == 3) {
                        double dc = (double)(int64_t)raw;
                        memcpy(&v, &dc, 8);
                    }
                    wv[i] = v;
                }
                if (ABS && did - hb < win) {
                    /* lean absorb: compile-time field walk, uniform ops */
                    uint32_t rel = did - hb;
                    atomicAdd(&ltou[rel], 1u);
                    uint32_t bse = rel * (uint32_t)(NAR + NF);
                    #pragma unroll
                    for (int i = 0; i < NAR; i++) {
                        uint64_t v = prm.nsub[i] + (uint64_t)nf[i].d[j];
                        uint64_t* lv = &lval[bse + prm.naslot[i]];
                        if (prm.nop[i] == 0)
                            atomicAdd((unsigned long long*)lv,
                                      (unsigned long long)v);
                        else if (prm.nop[i] == 1)
                            atomicMax((unsigned long long*)lv,
                                      (unsigned long long)v);
                        else
                            atomicMax((unsigned long long*)lv,
                                      (unsigned long long)~v);
                    }
                    #pragma unroll
                    for (int i = 0; i < NF; i++) {
                        uint64_t* lv = &lval[bse + prm.waslot[i]];
                        if (prm.wop[i] == 0) {
                            double dd2;
                            memcpy(&dd2, &wv[i], 8);
                            atomic_add_f64_lds(lv, dd2);
                        } else if (prm.wop[i] == 1)
                            atomicAdd((unsigned long long*)lv,
                                      (unsigned long long)wv[i]);
                        else if (prm.wop[i] == 2)
                            atomicMax((unsigned long long*)lv,
                                      (unsigned long long)wv[i]);
                        else
                            atomicMax((unsigned long long*)lv,
                                      (unsigned long long)~wv[i]);
                    }
                    continue;
                }
                uint32_t b = did >> ds.shift;
                if (PK) {
                    /* split store: one u32 hdr + NF aligned payload words */
                    uint32_t hw = did << lay.pkdidsh;
                    #pragma unroll
                    for (int i = 0; i < NAR; i++)
                        hw |= nf[i].d[j] << lay.pksh[i];
                    uint32_t pos = atomicAdd(&lcur[b], 1u);
                    hdr[pos] = hw;
                    uint64_t* dst = rec + (size_t)pos * NF;
                    typedef long long ll2 __attribute__((ext_vector_type(2)));
                    #pragma unroll
                    for (int w = 0; w + 1 < NF; w += 2) {
                        ll2 v;
                        v.x = (long long)wv[w];
                        v.y = (long long)wv[w + 1];
                        *(ll2*)&dst[w] = v;
                    }
                    if (NF & 1) dst[NF - 1] = wv[NF - 1];
                    continue;
                }
                uint64_t regs[NWORDS];
                #pragma unroll
                for (int w = 0; w < NWORDS; w++) regs[w] = 0;
                regs[0] = did;
                #pragma unroll
                for (int i = 0; i < NAR; i++) {
                    uint64_t f = nf[i].d[j];
                    if ((1 + i) & 1) regs[(1 + i) >> 1] |= f << 32;
                    else             regs[(1 + i) >> 1] |= f;
                }
                #pragma unroll
                for (int i = 0; i < NF; i++) regs[WOFF + i] = wv[i];
                uint32_t pos = atomicAdd(&lcur[b], 1u);
                /* compile-time-width stores (regs never becomes a pointer) */
                uint64_t* dst = rec + (size_t)pos * NWORDS;
                typedef long long ll2 __attribute__((ext_vector_type(2)));
                #pragma unroll
                for (int w = 0; w < NWORDS; w += 2) {
                    if (w + 1 < NWORDS) {
                        ll2 v;
                        v.x = (long long)regs[w];
                        v.y = (long long)regs[w + 1];
                        *(ll2*)&dst[w] = v;
                    } else {
                        dst[w] = regs[w];
                    }
                }
            }
        }
    }
    if (ABS) {   /* stream the block's hot-bucket LDS array to its slab:
                    coalesced plain stores, zero atomics; k_dabs_reduce
                    folds slabs into gvals/gtouch */
        __syncthreads();
        uint64_t* vs = vslab + (size_t)blockIdx.x * win * nv;
        uint32_t* ts = tslab + (size_t)blockIdx.x * win;
        for (uint32_t i = threadIdx.x; i < win * (uint32_t)nv; i += BS)
            vs[i] = lval[i];
        for (uint32_t i = threadIdx.x; i < win; i += BS) ts[i] = ltou[i];
    }
}

/* fold the ABS slabs into the dense global accumulators. For a fixed slab b
 * consecutive threads read consecutive addresses (coalesced); the per-slot
 * combine follows ds.vop exactly as k_dagg's flush (0 identity for add and
 * for max-of-encoding). One atomic per live slot per value word. */
__global__ void k_dabs_reduce(DenseSpec ds, uint32_t hb, uint32_t nblocks,
                              const uint64_t* vslab, const uint32_t* tslab,
                              uint64_t* gvals, uint64_t* gtouch) {
    const uint32_t win = 1u << ds.shift;
    const int nv = ds.nv;
    uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t sl = tid; sl < win; sl += gs) {
        uint64_t t = 0;
        for (uint32_t b = 0; b < nblocks; b++)
            t += tslab[(size_t)b * win + sl];
        if (t)
            atomicAdd((unsigned long long*)&gtouch[hb + sl],
                      (unsigned long long)t);
    }
    for (uint64_t i = tid; i < (uint64_t)win * nv; i += gs) {
        uint32_t v = (uint32_t)(i % nv);
        uint32_t sl = (uint32_t)(i / nv);
        uint64_t* g = &gvals[((uint64_t)hb + sl) * nv + v];
        if (ds.vop[v] == 1) {
            double acc = 0;
            for (uint32_t b = 0; b < nblocks; b++) {
                uint64_t x = vslab[(size_t)b * win * nv + i];
                double dd;
                memcpy(&dd, &x, 8);
                acc += dd;
            }
            if (acc != 0.0) atomic_add_f64_global(g, acc);
        } else if (ds.vop[v] == 2) {
            uint64_t acc = 0;
            for (uint32_t b = 0; b < nblocks; b++) {
                uint64_t x = vslab[(size_t)b * win * nv + i];
                acc = acc > x ? acc : x;
            }
            if (acc)
                atomicMax((unsigned long long*)g, (unsigned long long)acc);
        } else {
            uint64_t acc = 0;
            for (uint32_t b = 0; b < nblocks; b++)
                acc += vslab[(size_t)b * win * nv + i];
            if (acc)
                atomicAdd((unsigned long long*)g, (unsigned long long)acc);
        }
    }
}

/* pass 3: per-descriptor dense LDS aggregation. LDS carve:
 * [ 2^shift * nv value u64 ][ 2^shift touched u32 ]. Direct ds-atomics at
 * lidx — no claims, no flush generations; one flush per descriptor.
 * ILP=2 keeps two records' load->ds-atomic chains in flight per lane. */
template <int BS, int ILP = 1, bool PK = false>
__global__ void __launch_bounds__(BS)
k_dagg(BkQuerySpec q, DenseSpec ds, DRecLayout lay, const uint64_t* rec,
       const uint32_t* hdr, const DDesc* descs, uint32_t ndesc,
       uint64_t* gvals, uint64_t* gtouch) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t sig = 1u << ds.shift;
    const int nv = ds.nv;
    uint64_t* lval = lds;
    uint32_t* ltou = (uint32_t*)(lds + (size_t)sig * nv);
    for (uint32_t d = blockIdx.x; d < ndesc; d += gridDim.x) {
        DDesc de = descs[d];
        for (uint32_t i = threadIdx.x; i < sig * (uint32_t)nv; i += BS)
            lval[i] = 0;
        for (uint32_t i = threadIdx.x; i < sig; i += BS) ltou[i] = 0;
        __syncthreads();
        uint32_t dbase = de.bucket << ds.shift;
        uint64_t end = de.start + de.cnt;
        for (uint64_t i = de.start + threadIdx.x; i < end;
             i += (uint64_t)BS * ILP) {
            if (PK) {
                dagg_rec_pk(q, ds, lay, hdr[i],
                            rec + i * (uint64_t)lay.pknf, dbase, lval, ltou,
                            nv);
                if (ILP == 2 && i + BS < end)
                    dagg_rec_pk(q, ds, lay, hdr[i + BS],
                                rec + (i + BS) * (uint64_t)lay.pknf, dbase,
                                lval, ltou, nv);
            } else {
                dagg_rec(q, ds, lay, rec + i * (uint64_t)lay.nwords, dbase,
                         lval, ltou, nv);
                if (ILP == 2 && i + BS < end)
                    dagg_rec(q, ds, lay,
                             rec + (i + BS) * (uint64_t)lay.nwords, dbase,
                             lval, ltou, nv);
            }
        }
        __syncthreads();
        for (uint32_t sl = threadIdx.x; sl < sig; sl += BS) {
            uint32_t t = ltou[sl];
            if (!t) continue;
            uint32_t did = dbase + sl;
            atomicAdd((unsigned long long*)&gtouch[did],
                      (unsigned long long)t);
            for (int v = 0; v < nv; v++) {
                uint64_t x = lval[(size_t)sl * nv + v];
                if (!x) continue;   /* identity for add / max-of-encoding */
                uint64_t* g = &gvals[(size_t)did * nv + v];
                switch (ds.vop[v]) {
                    case 0:
                        atomicAdd((unsigned long long*)g,
                                  (unsigned long long)x);
                        break;
                    case 1: {
                        double dd;
                        memcpy(&dd, &x, 8);
                        atomic_add_f64_global(g, dd);
                        break;
                    }
                    default:
                        atomicMax((unsigned long long*)g,
                                  (unsigned long long)x);
                        break;
                }
            }
        }
        __syncthreads();
    }
}

/* live-group count over the dense touched array */
__global__ void k_dcount(const uint64_t* gtouch, uint64_t span,
                         uint64_t* out) {
    uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    uint64_t mine = 0;
    for (uint64_t did = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         did < span; did += gs)
        mine += gtouch[did] != 0;
    for (int off = 32; off > 0; off >>= 1)
        mine += __shfl_down((unsigned long long)mine, off, 64);
    if ((threadIdx.x & 63) == 0)
        atomicAdd((unsigned long long*)out, (unsigned long long)mine);
}

/* compact the dense result arrays DIRECTLY into the wire blob (the hash
 * table is never built on this path): keys reconstruct from the dense id,
 * per-agg states synthesize exactly as agg_update_slot would have built
 * them — COUNT values and non-null counts are the touched counter
 * (dense_spans guarantees non-nullable inputs). */
__global__ void k_dcompact(BkQuerySpec q, DenseSpec ds, const uint64_t* gvals,
                           const uint64_t* gtouch, uint64_t* counter,
                           uint32_t* out_flags, uint64_t* out_k0,
                           uint64_t* out_k1, uint64_t* out_states,
                           uint64_t cap) {
    const int nst = 2 * q.n_aggs;
    uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t did = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         did < ds.span; did += gs) {
        uint64_t t = gtouch[did];
        if (!t) continue;
        uint64_t i = atomicAdd((unsigned long long*)counter, 1ull);
        if (i >= cap) continue;
        out_flags[i] = 0;
        out_k0[i] = ds.base0 + (did >> ds.k1bits);
        out_k1[i] = q.n_group >= 2
                        ? ds.base1 + (did & ((1ull << ds.k1bits) - 1))
                        : 0;
        uint64_t* st = out_states + i * (uint64_t)nst;
        for (int32_t a = 0; a < q.n_aggs; a++) {
            int at = q.aggs[a].agg_type;
            if (at == BK_AGG_COUNT_STAR || at == BK_AGG_COUNT) {
                st[2 * a] = t;      /* cnt word 0, as in agg_update_slot */
                st[2 * a + 1] = 0;
                continue;
            }
            st[2 * a] = gvals[did * (uint64_t)ds.nv + ds.vslot[a]];
            st[2 * a + 1] = t;
        }
    }
}

/* ---- host side ---- */

static int ceil_log2_u64(uint64_t x) {
    int b = 0;
    while ((1ull << b) < x && b < 63) b++;
    return b;
}

typedef decltype(&k_dhisto<512, false, false, 0>) DHistoFn;
typedef decltype(&k_dscatter<512, false>) DScatFn;
typedef decltype(&k_dscatter_e<512, 1, 0, 0, false>) DScatEFn;
typedef decltype(&k_dagg<1024, 1>) DAggFn;

/* launch plan of the dense route (run_dense), fixed once per call like the
 * hash route's PartPlan. Every knob of the route is read in dense_plan (and
 * the helpers it calls once each) and nowhere else. */
struct DensePlan {
    int pref;                   /* BK_DENSE: 0 never; below 1 the sorted path
                                 * goes first (sorted_first) */
    DenseSpec ds;
    DRecLayout lay;             /* final: PACK32 split decided */
    bool simple;
    BkQuerySpec qpad;
    const BkQuerySpec* qk;      /* SIMPLE: the padded copy (points into this
                                 * plan: plans are not copied) */
    int nblocks, threads;       /* histo + scatter grid and block shape */
    DHistoFn histo_fn;
    DScatFn scat_fn;            /* masked scatter, when no eager plan holds */
    DScatEFn scat_e, scat_abs;  /* eager scatter, its absorbing twin, or null */
    DScatE eprm;
    DAggFn dagg_fn;
    size_t histo_lds, scat_lds, abs_lds, dagg_lds;
    bool dabs_on;               /* BK_DABS: chunks may absorb a hot bucket... */
    double dabs_min;            /* ...holding this share of their survivors */
    size_t abs_win;             /* dense ids per bucket = absorb window */
    int pipe;                   /* BK_DPIPE in 1..4; 0 = unset (by size) */
    uint64_t dagg_chunk;        /* records per dagg descriptor; 0 = by count */
    uint32_t dagg_grid;         /* dagg grid cap */
    DensePlan() = default;
    DensePlan(const DensePlan&) = delete;
};

/* Eligibility and id spans: 1-2 fn-free non-nullable keys whose dense ids
 * fit BK_DENSE_MAX (default 2^23), and non-nullable plain aggregate inputs
 * (counts synthesize from `touched`). */
static bool dense_spans(BkgTable* t, const BkQuerySpec* q, DenseSpec* ds,
                        uint64_t* span_out) {
    if (q->n_group < 1 || q->n_group > 2) return false;
    if (any_group_bits(q)) return false;
    for (int32_t k = 0; k < q->n_group; k++) {
        if (q->group_fns[k]) return false;
        if (t->valid[q->group_cols[k]]) return false;
    }
    for (int32_t a = 0; a < q->n_aggs; a++) {
        int at = q->aggs[a].agg_type;
        if (at == BK_AGG_COUNT_STAR) continue;
        if (at != BK_AGG_COUNT && at != BK_AGG_SUM && at != BK_AGG_AVG &&
            at != BK_AGG_MIN && at != BK_AGG_MAX)
            return false;                      /* distinct kinds: hash path */
        if (q->aggs[a].prog_len > 0) return false;  /* validity unknown */
        int col = q->aggs[a].col;
        if (col < 0 || t->valid[col]) return false;
        if (q->aggs[a].arith &&
            (q->aggs[a].col2 < 0 || t->valid[q->aggs[a].col2]))
            return false;
    }
    uint64_t cap = 1ull << 23;
    if (const char* e = getenv("BK_DENSE_MAX")) cap = (uint64_t)atoll(e);
    uint64_t kspan[2] = {0, 0};
    for (int32_t k = 0; k < q->n_group; k++) {
        int c = q->group_cols[k];
        if (ensure_stats(t, c) != 0 || !t->stat_ok[c] ||
            t->stat_max[c] < t->stat_min[c])
            return false;
        kspan[k] = t->stat_max[c] - t->stat_min[c];
        if (kspan[k] >= cap) return false;
    }
    const bool two = q->n_group == 2;
    ds->base0 = t->stat_min[q->group_cols[0]];
    ds->base1 = two ? t->stat_min[q->group_cols[1]] : 0;
    ds->k1bits = two ? (uint32_t)ceil_log2_u64(kspan[1] + 1) : 0;
    uint64_t span = (kspan[0] + 1) << ds->k1bits;
    if (ds->k1bits >= 24 || span > cap) return false;
    ds->span = (uint32_t)span;
    *span_out = span;
    return true;
}

/* record layout (unsplit) and ds's value slots: narrow u32 deltas for
 * int64-ish inputs whose span fits, wide u64 otherwise; u32 fields first (did
 * at offset 0), pad, then 8-byte-aligned wide fields. False past 8 words. */
static bool dense_rec_layout(BkgTable* t, const BkQuerySpec* q, DenseSpec* ds,
                             DRecLayout* lay) {
    int nv = 0;
    int nwide = 0;
    lay->pk = 0;                               /* dense_pack32 may split it */
    int kind[BK_MAX_AGGS];                     /* 0 none, 1 narrow, 2 wide */
    for (int32_t a = 0; a < q->n_aggs; a++) {
        int at = q->aggs[a].agg_type;
        lay->off32[a] = -1;
        lay->wide[a] = 0;
        lay->vbase[a] = 0;
        ds->vslot[a] = -1;
        kind[a] = 0;
        if (at == BK_AGG_COUNT_STAR || at == BK_AGG_COUNT) continue;
        bool is_f64 = q->agg_in_types[a] == BK_DOUBLE || at == BK_AGG_AVG;
        bool narrow = false;
        uint64_t vbase = 0;
        if (!is_f64 && !q->aggs[a].arith) {
            int col = q->aggs[a].col;
            if (ensure_stats(t, col) == 0 && t->stat_ok[col] &&
                t->stat_max[col] >= t->stat_min[col] &&
                t->stat_max[col] - t->stat_min[col] < 0xFFFFFFFFull) {
                narrow = true;
                /* SUM accumulates values, MIN/MAX accumulate encodings —
                 * both spans equal the encoding span (monotonic) */
                const uint64_t sign =
                    q->agg_in_types[a] == BK_STRING ? 0 : 1ull << 63;
                vbase = t->stat_min[col] ^ (at == BK_AGG_SUM ? sign : 0);
            }
        }
        kind[a] = narrow ? 1 : 2;
        lay->vbase[a] = vbase;
        ds->vslot[a] = nv;
        ds->vop[nv] = (at == BK_AGG_MIN || at == BK_AGG_MAX) ? 2
                      : is_f64                               ? 1
                                                             : 0;
        nv++;
        if (!narrow) nwide++;
    }
    ds->nv = nv;
    int off = 1;                               /* u32 slot 0 = did */
    for (int32_t a = 0; a < q->n_aggs; a++)
        if (kind[a] == 1) { lay->off32[a] = off++; }
    if (nwide > 0 && (off & 1)) off++;         /* align wide fields */
    for (int32_t a = 0; a < q->n_aggs; a++)
        if (kind[a] == 2) { lay->off32[a] = off; lay->wide[a] = 1; off += 2; }
    lay->nwords = (off + 1) / 2;
    return lay->nwords <= 8;
}

/* bucket granularity: largest power-of-2 slots/bucket whose LDS carve
 * (nv u64 values + u32 touched per slot) fits 64 KB — 2 dagg blocks/CU
 * (and headroom for a co-resident scatter block in the pipelined run);
 * BK_DAGG_SHIFT overrides. False past 4096 buckets (histo arrays). */
static bool dense_bucket_shift(DenseSpec* ds, uint64_t span) {
    const size_t slot = 8 * (size_t)ds->nv + 4;
    uint32_t shift = 14;
    while (shift > 0 && (size_t)(1u << shift) * slot > 64 * 1024) shift--;
    if (const char* e = getenv("BK_DAGG_SHIFT")) {
        int v = atoi(e);
        if (v >= 6 && v <= 14 && (size_t)(1u << v) * slot <= 144 * 1024)
            shift = (uint32_t)v;
    }
    ds->shift = shift;
    ds->P = (uint32_t)((span + (1ull << shift) - 1) >> shift);
    ds->hshift = ds->shift >= ds->k1bits ? ds->shift - ds->k1bits
                                         : 0xFFFFFFFFu;
    return ds->P <= 4096;
}

/* classify the record fields for the eager scatter; false => masked path */
static bool dense_eager_plan(const DevCols& dc, const BkQuerySpec* q,
                             const DenseSpec& ds, const DRecLayout& lay,
                             DScatE* prm, int* nar_out, int* nf_out) {
    int nar = 0, nf = 0;
    constexpr int WMAX = 3, NMAX = 2;
    for (int32_t k = 0; k < q->n_group; k++) {
        const DevCol& c = dc.c[q->group_cols[k]];
        if (c.lshift > 2 || c.type == BK_DOUBLE) return false;
    }
    int nu32 = 1;
    for (int32_t a = 0; a < q->n_aggs; a++) {
        if (lay.off32[a] < 0) continue;
        if (q->aggs[a].arith || q->aggs[a].prog_len > 0) return false;
        int col = q->aggs[a].col;
        const DevCol& c = dc.c[col];
        int at = q->aggs[a].agg_type;
        if (!lay.wide[a]) {
            if (nar >= NMAX || c.lshift > 2) return false;
            if (lay.off32[a] != nu32) return false;  /* canonical order */
            prm->ncol[nar] = col;
            /* SUM fields are value-domain deltas (no flip); MIN/MAX fields
             * are encoding deltas (int flip; STRING codes pass through) */
            prm->nflip[nar] = (at == BK_AGG_MIN || at == BK_AGG_MAX) &&
                                      c.type != BK_STRING
                                  ? (1ull << 63)
                                  : 0;
            prm->nsub[nar] = lay.vbase[a];
            prm->naslot[nar] = ds.vslot[a];
            prm->nop[nar] = at == BK_AGG_MAX ? 1 : at == BK_AGG_MIN ? 2 : 0;
            nar++;
            nu32++;
        } else {
            if (nf >= WMAX || c.lshift != 3) return false;
            prm->wcol[nf] = col;
            int wm = 0;
            if (at == BK_AGG_MIN || at == BK_AGG_MAX)
                wm = c.type == BK_DOUBLE ? 2 : 1;
            else if (at == BK_AGG_AVG && c.type != BK_DOUBLE)
                wm = 3;   /* AVG over a wide int64 column: the aggregate
                             state is f64 (agg_fn_call.cpp input cast) —
                             convert in-kernel; raw bits would be garbage */
            prm->wmode[nf] = wm;
            prm->waslot[nf] = ds.vslot[a];
            prm->wop[nf] = at == BK_AGG_MIN   ? 3
                           : at == BK_AGG_MAX ? 2
                           : (c.type == BK_DOUBLE || at == BK_AGG_AVG) ? 0
                                                                       : 1;
            nf++;
        }
    }
    /* canonical wide offsets */
    int woff2 = ((nu32 + 1) / 2) * 2;
    int wi = 0;
    for (int32_t a = 0; a < q->n_aggs; a++) {
        if (lay.off32[a] < 0 || !lay.wide[a]) continue;
        if (lay.off32[a] != woff2 + 2 * wi) return false;
        wi++;
    }
    int nwords = nf > 0 ? woff2 / 2 + nf : (nu32 + 1) / 2;
    if (nwords != lay.nwords) return false;
    *nar_out = nar;
    *nf_out = nf;
    return true;
}

static DScatEFn pick_dscat_e(int nk, int nar, int nf, bool abs_,
                             bool pk = false) {
    #define DSE(K, A, F) \
        if (nk == K && nar == A && nf == F) \
            return pk     ? k_dscatter_e<512, K, A, F, false, true> \
                   : abs_ ? k_dscatter_e<512, K, A, F, true> \
                          : k_dscatter_e<512, K, A, F, false>;
    DSE(1, 0, 0) DSE(1, 0, 1) DSE(1, 0, 2) DSE(1, 0, 3)
    DSE(1, 1, 0) DSE(1, 1, 1) DSE(1, 1, 2) DSE(1, 1, 3)
    DSE(1, 2, 0) DSE(1, 2, 1) DSE(1, 2, 2) DSE(1, 2, 3)
    DSE(2, 0, 0) DSE(2, 0, 1) DSE(2, 0, 2) DSE(2, 0, 3)
    DSE(2, 1, 0) DSE(2, 1, 1) DSE(2, 1, 2) DSE(2, 1, 3)
    DSE(2, 2, 0) DSE(2, 2, 1) DSE(2, 2, 2) DSE(2, 2, 3)
    #undef DSE
    return nullptr;
}

/* PACK32 split records (see DRecLayout): possible when did bits + every
 * narrow field's stats bits fit one u32 (stats are exact min/max, so field
 * deltas provably fit). Fills the pk fields of lay; false leaves it unsplit.
 * MEASURED-DEAD as default (DESIGN.md: 17.51 ms packed vs 16.60 ms AoS, the
 * scatter is store-latency-bound, not byte-bound). BK_DREC_PACK=1 opts in;
 * parity tests force it. */
static bool dense_pack32(const BkgTable* t, const DenseSpec& ds,
                         const DScatE& eprm, int nar, int nf, DRecLayout* lay) {
    int bits[2] = {0, 0};
    int tot = 0;
    for (int i = 0; i < nar; i++) {
        int col = eprm.ncol[i];
        if (!t->stat_ok[col]) return false;
        bits[i] = ceil_log2_u64(t->stat_max[col] - t->stat_min[col] + 1);
        tot += bits[i];
    }
    if (ceil_log2_u64(ds.span) + tot > 32) return false;
    lay->pk = 1;
    lay->pknf = nf;
    lay->pkdidsh = (uint32_t)tot;
    lay->pksh[0] = nar == 2 ? (uint32_t)bits[1] : 0;
    lay->pksh[1] = 0;
    for (int i = 0; i < 2; i++)
        lay->pkmask[i] = bits[i] >= 32 ? 0xFFFFFFFFu : ((1u << bits[i]) - 1u);
    return true;
}

/* false for a shape the dense route does not take (plan left undefined) */
static bool dense_plan(DensePlan* pl, BkgTable* t, const BkQuerySpec* q) {
    pl->pref = 1;
    if (const char* e = getenv("BK_DENSE")) pl->pref = atoi(e);
    if (pl->pref == 0) return false;
    DenseSpec& ds = pl->ds;
    uint64_t span = 0;
    if (!dense_spans(t, q, &ds, &span) ||
        !dense_rec_layout(t, q, &ds, &pl->lay) ||
        !dense_bucket_shift(&ds, span))
        return false;

    pl->nblocks = 4096;
    if (const char* e = getenv("BK_DPART_BLOCKS")) pl->nblocks = atoi(e);
    if (pl->nblocks < 1) pl->nblocks = 4096;    /* no zero-block launch */
    pl->threads = 512;
    DevCols dc = table_cols(t);

    const bool simple = pl->simple =
        query_simple(t, q) && getenv("BK_NO_SIMPLE") == nullptr;
    pl->qk = q;
    if (simple) { pl->qpad = pad_simple_q(q); pl->qk = &pl->qpad; }
    bool vec = simple;
    if (vec)
        for (int j = 0; j < 4; j++)
            if (dc.c[pl->qpad.conjuncts[j].col].lshift > 2) vec = false;
    /* eager bucket keys: key col(s) vector-loadable */
    int kv = 0;
    if (vec) {
        const DevCol& c0 = dc.c[q->group_cols[0]];
        bool k0ok = c0.lshift <= 2 && c0.type != BK_DOUBLE;
        if (ds.hshift != 0xFFFFFFFFu) {
            kv = k0ok ? 1 : 0;
        } else if (q->n_group >= 2) {
            const DevCol& c1 = dc.c[q->group_cols[1]];
            kv = (k0ok && c1.lshift <= 2 && c1.type != BK_DOUBLE) ? 2 : 0;
        }
    }
    /* <=2 real conjuncts: the NCJ=2 instantiation halves the predicate
     * loads (padding duplicates are AND-idempotent, so evaluating only
     * the first two is exact; tail tiles still use the 4-padded
     * row_passes) */
    bool cj2 = q->n_conjuncts <= 2;
    pl->histo_fn =
        kv == 2  ? (cj2 ? k_dhisto<512, true, true, 2, 2>
                        : k_dhisto<512, true, true, 2, 4>)
        : kv == 1 ? (cj2 ? k_dhisto<512, true, true, 1, 2>
                         : k_dhisto<512, true, true, 1, 4>)
        : vec     ? (cj2 ? k_dhisto<512, true, true, 0, 2>
                         : k_dhisto<512, true, true, 0, 4>)
        : simple  ? k_dhisto<512, true, false, 0>
                  : k_dhisto<512, false, false, 0>;
    pl->scat_fn = simple ? k_dscatter<512, true> : k_dscatter<512, false>;
    pl->histo_lds = 8 + (size_t)ds.P * 4;
    pl->scat_lds = (size_t)ds.P * 4;

    /* eager scatter needs no SIMPLE query shape — the predicate was already
     * settled into passbits; only the field classification matters.
     * BK_NO_DEAGER keeps the masked scatter: no absorb, no PACK32 either. */
    memset(&pl->eprm, 0, sizeof pl->eprm);
    int nar = 0, nf = 0;
    const bool eager = getenv("BK_NO_DEAGER") == nullptr &&
                       dense_eager_plan(dc, q, ds, pl->lay, &pl->eprm, &nar, &nf);
    pl->scat_e = eager ? pick_dscat_e(q->n_group, nar, nf, false) : nullptr;
    pl->scat_abs = eager ? pick_dscat_e(q->n_group, nar, nf, true) : nullptr;

    /* hot-bucket absorption gate (per chunk; see k_dscatter_e ABS): the
     * measured per-bucket survivor histogram decides. LDS carve must fit
     * beside the bucket cursors; dabs_min = share of a chunk's survivors the
     * hottest bucket must hold. MEASURED-DEAD as default (DESIGN.md: dagg
     * 3.78 -> 2.27 ms, but the scatter pays 12.6 -> 16.0 ms); bit-identical
     * either way; BK_DABS=1 opts in (and the parity tests force it). */
    pl->dabs_min = 0.15;
    if (const char* e = getenv("BK_DABS_MIN")) pl->dabs_min = atof(e);
    pl->abs_win = (size_t)1 << ds.shift;
    pl->dagg_lds = pl->abs_win * (8 * (size_t)ds.nv + 4);
    pl->abs_lds = pl->dagg_lds + (size_t)ds.P * 4;
    pl->dabs_on = pl->scat_e != nullptr && getenv("BK_DABS") &&
                  atoi(getenv("BK_DABS")) != 0 && pl->abs_lds <= 144 * 1024;

    /* absorb takes precedence: with it on, every chunk — absorbing or not —
     * runs the unsplit layout */
    bool pk = pl->scat_e && !pl->dabs_on && getenv("BK_DREC_PACK") &&
              atoi(getenv("BK_DREC_PACK")) != 0 &&
              dense_pack32(t, ds, pl->eprm, nar, nf, &pl->lay);
    if (pk) pl->scat_e = pick_dscat_e(q->n_group, nar, nf, false, true);

    int dilp = 2;
    if (const char* e = getenv("BK_DAGG_ILP")) dilp = atoi(e);
    pl->dagg_fn = pk ? (dilp == 2 ? k_dagg<1024, 2, true>
                                  : k_dagg<1024, 1, true>)
                     : (dilp == 2 ? k_dagg<1024, 2> : k_dagg<1024, 1>);
    pl->dagg_chunk = 0;
    if (const char* e = getenv("BK_DAGG_CHUNK")) pl->dagg_chunk = (uint64_t)atoll(e);
    pl->dagg_grid = 32768;
    if (const char* e = getenv("BK_DAGG_GRID")) {
        uint32_t g = (uint32_t)atoi(e);
        if (g > 0 && g < pl->dagg_grid) pl->dagg_grid = g;
    }
    pl->pipe = 0;
    if (const char* e = getenv("BK_DPIPE"))
        pl->pipe = std::min(4, std::max(1, atoi(e)));
    return true;
}

/* Dense GROUP BY for one attempt; returns like run_partitioned, whose chunk
 * scaffolding (bkgpu.hip) this loop shares. When piped, chunk c's
 * LDS-atomic-heavy dagg overlaps chunk c+1's HBM-bound histo/scatter; the
 * accumulators (gvals/gtouch) are SHARED — every op is an order-free atomic
 * (adds / maxes), so results are identical to the single pass. */
static int run_dense(BkgAggOut* o, BkgTable* t, const BkQuerySpec* q,
                     const DensePlan& pl, int64_t row_begin, int64_t row_end) {
    const DenseSpec& ds = pl.ds;
    const DRecLayout& lay = pl.lay;
    int64_t range = row_end - row_begin;
    if (range >= (int64_t)UINT32_MAX * DPART_T) {
        set_err("dense range too large");
        return -1;
    }
    int npipe = pl.pipe ? pl.pipe : range >= 400 * 1000 * 1000 ? 2 : 1;
    ChunkSplit sp(row_begin, row_end, npipe);
    if (sp.piped() && !sp.streams) return -1;
    DevCols dc = table_cols(t);
    const uint32_t P = ds.P;
    const int nblocks = pl.nblocks, threads = pl.threads;
    const uint64_t span_alloc = (uint64_t)P << ds.shift;

    struct Slot : ChunkBufs {
        uint16_t* passbits = nullptr;
        DDesc* ddesc = nullptr;
        uint64_t* vslab = nullptr;   /* ABS per-block hot-bucket slabs */
        uint32_t* tslab = nullptr;
        void recycle() { ChunkBufs::recycle(); pool_free(ddesc); ddesc = nullptr; }
    } sl[2];
    uint64_t *gvals = nullptr, *gtouch = nullptr;
    auto cleanup = [&]() {
        for (Slot& s : sl) {
            pool_free(s.passbits); pool_free(s.ddesc); pool_free(s.vslab);
            pool_free(s.tslab); s.release();
        }
        pool_free(gvals); pool_free(gtouch);
    };
    uint64_t per_tiles = (uint64_t)((sp.per + DPART_T - 1) / DPART_T);
    for (int i = 0; i < sp.nslots(); i++) {
        CHK("dense", pool_alloc((void**)&sl[i].passbits, per_tiles * 2 + 16));
        CHK("dense", sl[i].alloc_prefix(nblocks, P));
    }
    const size_t gvals_bytes = (size_t)span_alloc * ds.nv * 8 + 8;
    CHK("dense", pool_alloc((void**)&gvals, gvals_bytes));
    CHK("dense", pool_alloc((void**)&gtouch, (size_t)span_alloc * 8));
    CHK("dense", hipMemset(gvals, 0, gvals_bytes));
    CHK("dense", hipMemset(gtouch, 0, (size_t)span_alloc * 8));

    static const char* DNAMES[] = {"dhisto", "dtotals", "dscan", "doffs",
                                   "dscatter", "dagg", "dtotab"};
    ChunkClock ck{sp};
    CHK("dense", ck.start());
    ck.mark();
    std::vector<DDesc> descs;
    std::vector<uint32_t> h_tot(P), h_base(P);
    for (int c = 0; c < npipe; c++) {
        Chunk k;
        CHK("dense", chunk_open(sp, c, sl, &k));
        if (k.ce <= k.cb) break;
        Slot& s = sl[k.si];
        hipStream_t st = k.st;
        CHK("dense", hipMemsetAsync(s.totals, 0, (size_t)P * 4, st));
        hipLaunchKernelGGL(pl.histo_fn, dim3(nblocks), dim3(threads),
                           pl.histo_lds, st, dc, *pl.qk, ds, k.cb, k.ce,
                           s.passbits, s.H, s.totals, o->ctrs + 1);
        ck.mark();
        uint64_t total = 0;
        CHK("dense", prefix_pass(s, P, st, ck, &total,
                                 h_tot.data(), h_base.data()));
        /* hottest bucket of THIS chunk (measured counts; first of equals) */
        const uint32_t hotb = (uint32_t)(
            std::max_element(h_tot.begin(), h_tot.end()) - h_tot.begin());
        bool absorb = pl.dabs_on && total > 0 &&
                      h_tot[hotb] >= (uint64_t)(pl.dabs_min * (double)total);
        uint32_t* hdrp = nullptr;
        if (total > 0) {
            size_t rec_bytes = lay.pk
                ? (size_t)total * ((size_t)lay.pknf * 8 + 4) + 8
                : (size_t)total * lay.nwords * 8;
            CHK("dense", pool_alloc((void**)&s.rec, rec_bytes));
            if (lay.pk) hdrp = (uint32_t*)(s.rec + (size_t)total * lay.pknf);
            if (absorb) {
                const size_t slab = (size_t)nblocks * pl.abs_win;
                if (!s.vslab && ds.nv > 0)
                    CHK("dense", pool_alloc((void**)&s.vslab, slab * ds.nv * 8));
                if (!s.tslab)
                    CHK("dense", pool_alloc((void**)&s.tslab, slab * 4));
                hipLaunchKernelGGL(pl.scat_abs, dim3(nblocks), dim3(threads),
                                   pl.abs_lds, st, dc, *pl.qk, ds, lay,
                                   pl.eprm, k.cb, k.ce, s.passbits, s.H,
                                   s.base, s.rec, nullptr, hotb << ds.shift, s.vslab, s.tslab);
                hipLaunchKernelGGL(k_dabs_reduce, dim3(256), dim3(256), 0, st,
                                   ds, hotb << ds.shift, (uint32_t)nblocks,
                                   s.vslab, s.tslab, gvals, gtouch);
            } else if (pl.scat_e)
                hipLaunchKernelGGL(pl.scat_e, dim3(nblocks), dim3(threads),
                                   pl.scat_lds, st, dc, *pl.qk, ds, lay,
                                   pl.eprm, k.cb, k.ce, s.passbits, s.H,
                                   s.base, s.rec, hdrp, 0u, nullptr, nullptr);
            else
                hipLaunchKernelGGL(pl.scat_fn, dim3(nblocks), dim3(threads),
                                   pl.scat_lds, st, dc, *pl.qk, ds, lay, k.cb,
                                   k.ce, s.passbits, s.H, s.base, s.rec);
        }
        ck.mark();
        /* descriptors: per bucket, runs of <= CH records (balances skewed
         * range buckets); flush traffic = ndesc x live slots */
        uint64_t CH = pl.dagg_chunk ? pl.dagg_chunk
                                    : std::max<uint64_t>(65536, total / 768);
        descs.clear();
        for (uint32_t b = 0; b < P; b++) {
            if (absorb && b == hotb) continue;   /* records never written */
            uint64_t n = h_tot[b], s0 = h_base[b];
            for (uint64_t ofs = 0; ofs < n; ofs += CH)
                descs.push_back({b, (uint32_t)std::min<uint64_t>(CH, n - ofs),
                                 s0 + ofs});
        }
        if (total > 0 && !descs.empty()) {
            const size_t dbytes = descs.size() * sizeof(DDesc);
            CHK("dense", pool_alloc((void**)&s.ddesc, dbytes));
            CHK("dense", hipMemcpyAsync(s.ddesc, descs.data(), dbytes,
                                        hipMemcpyHostToDevice, st));
            uint32_t grid =
                (uint32_t)std::min<size_t>(descs.size(), pl.dagg_grid);
            hipLaunchKernelGGL(pl.dagg_fn, dim3(grid), dim3(1024), pl.dagg_lds,
                               st, *q, ds, lay, s.rec, hdrp, s.ddesc,
                               (uint32_t)descs.size(), gvals, gtouch);
        }
        ck.mark();
        CHK("dense", hipGetLastError());
    }
    ck.mark();                      /* "dtotab": nothing left to convert */
    CHK("dense", ck.finish(o, DNAMES, "dpipe"));
    /* adopt the dense result: compact reads these arrays directly; the
     * hash table (16-slot stub) is rebuilt lazily by dense_to_hash only
     * if merge/rollup need slot probing */
    pool_free(o->dvals);
    pool_free(o->dtouch);
    o->dvals = gvals;
    o->dtouch = gtouch;
    gvals = gtouch = nullptr;
    DenseSpec* spec = (DenseSpec*)malloc(sizeof(DenseSpec));
    *spec = ds;
    free(o->dense_spec);
    o->dense_spec = spec;
    o->dense_mode = true;
    cleanup();
    return 0;
}

/* compact the dense arrays straight into the wire blob (replaces the
 * k_compact path for dense_mode results; same blob layout) */
static int dense_compact(BkgAggOut* o) {
    if (!o->dirty && o->ngroups >= 0) return 0;
    DenseSpec* ds = (DenseSpec*)o->dense_spec;
    const int naggs = o->q.n_aggs;
    double t0 = debug_timing() ? now_ms() : 0;
    uint64_t ctr_host[3];
    HIP_CHECK(hipMemcpy(ctr_host, o->ctrs, 24, hipMemcpyDeviceToHost));
    double t1 = debug_timing() ? now_ms() : 0;
    o->rows_passed = (int64_t)ctr_host[1];
    HIP_CHECK(hipMemset(o->ctrs + 2, 0, 8));
    hipLaunchKernelGGL(k_dcount, dim3(1024), dim3(256), 0, 0,
                       o->dtouch, (uint64_t)ds->span, o->ctrs + 2);
    HIP_CHECK(hipGetLastError());
    uint64_t live = 0;
    HIP_CHECK(hipMemcpy(&live, o->ctrs + 2, 8, hipMemcpyDeviceToHost));
    if (debug_timing())
        fprintf(stderr, "[bkgpu] dcompact: ctr %.2f dcount %.2f ms\n",
                t1 - t0, now_ms() - t1);
    int64_t cap = live > 0 ? (int64_t)live : 1;
    if (o->blob) { pool_free(o->blob); o->blob = nullptr; }
    HIP_CHECK(pool_alloc((void**)&o->blob, blob_bytes_for(naggs, cap)));
    o->blob_groups = cap;
    HIP_CHECK(hipMemset(o->ctrs + 2, 0, 8));
    uint32_t* flags = (uint32_t*)o->blob;
    uint64_t* k0 = (uint64_t*)(flags + cap);
    uint64_t* k1 = k0 + cap;
    uint64_t* states = k1 + cap;
    hipLaunchKernelGGL(k_dcompact, dim3(2048), dim3(256), 0, 0,
                       o->q, *ds, o->dvals, o->dtouch, o->ctrs + 2,
                       flags, k0, k1, states, (uint64_t)cap);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(ctr_host, o->ctrs, 24, hipMemcpyDeviceToHost));
    o->ngroups = (int64_t)ctr_host[2] < cap ? (int64_t)ctr_host[2] : cap;
    o->dirty = false;
    return 0;
}

static int merge_blob_into(BkgAggOut* o, const void* blob, int64_t n_groups);

/* materialize a dense result as a hash table (for merge / rollup): compact
 * to the blob, allocate the table at the real size, re-insert. Results are
 * identical — the blob state array IS the table's state array. */
static int dense_to_hash(BkgAggOut* o) {
    if (!o->dense_mode) return 0;
    if (dense_compact(o) != 0) return -1;
    uint64_t rows_passed = (uint64_t)o->rows_passed;
    agg_release_table(o);
    int64_t nslots = next_pow2(std::max<int64_t>(o->ngroups * 2, 1024));
    if (agg_alloc(o, nslots) != 0) return -1;
    HIP_CHECK(hipMemcpy(o->ctrs + 1, &rows_passed, 8, hipMemcpyHostToDevice));
    o->dense_mode = false;
    pool_free(o->dvals);
    pool_free(o->dtouch);
    o->dvals = nullptr;
    o->dtouch = nullptr;
    free(o->dense_spec);
    o->dense_spec = nullptr;
    if (o->ngroups > 0 && merge_blob_into(o, o->blob, o->ngroups) != 0)
        return -1;
    return 0;
}
