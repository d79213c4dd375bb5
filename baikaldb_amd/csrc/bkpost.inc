// bkpost.inc — post-aggregation bridge: a finished aggregate materialized as
// an HBM-resident BkgTable of FINALIZED values, so HAVING (the filter),
// ORDER BY/LIMIT (top-N), window functions and re-aggregation run over
// GROUP BY output with the kernels they already have. Included from
// bkgpu.hip (shares BkgTable / BkgAggOut / agg_compact, bkprim.inc and the
// table-column helpers).
//
// Source: the compact wire blob (agg_compact) — every result form (hash
// table, dense arrays, sort-dedup table, scalar slot 0) settles into it, so
// nothing here is per-form:
//   [ flags: u32 * c ][ k0: u64 * c ][ k1: u64 * c ][ states: u64 * c*2*naggs ]
// Keys and states are read with the helpers bkgpu_agg_fetch uses
// (bk_keylayout.h: bk_key_get, bk_agg_finalize), so the two cannot drift.

#define POST_MAX_COLS (BK_MAX_GROUP + BK_MAX_AGGS)

/* by-value kernel arguments: walked ONLY with compile-time indices inside
 * fully unrolled loops (no runtime indexing into kernarg-resident arrays,
 * DESIGN §4/§6) */
struct PostTypes {
    int32_t key_type[BK_MAX_GROUP];   /* OUTPUT column type of each key */
    int32_t agg_type[BK_MAX_AGGS];
    int32_t in_type[BK_MAX_AGGS];
};
struct PostCols {
    void*    data[POST_MAX_COLS];     /* int32 (BK_STRING) or 8-byte cells */
    uint8_t* valid[POST_MAX_COLS];    /* null for COUNT-shaped columns */
};

/* store one finalized cell; returns the wave's "saw a NULL" as a bool */
__device__ __forceinline__ bool post_store(void* data, uint8_t* valid,
                                           int32_t type, int64_t i, bool live,
                                           bool has, uint64_t bits64) {
    if (live) {
        if (type == BK_STRING) ((int32_t*)data)[i] = has ? (int32_t)(uint32_t)bits64 : 0;
        else ((uint64_t*)data)[i] = has ? bits64 : 0;
        if (valid) valid[i] = has ? 1 : 0;
    }
    return __ballot(live && !has) != 0;
}

/* one thread per OUTPUT row i; reads group g = perm[i] (g = i when perm is
 * null) and writes every output column coalesced. nullmask: bit c set <=>
 * column c holds at least one NULL (one atomic per wave). */
__global__ void __launch_bounds__(256)
k_agg_finalize(const uint32_t* __restrict__ flags,
               const uint64_t* __restrict__ k0,
               const uint64_t* __restrict__ k1,
               const uint64_t* __restrict__ states,
               const uint32_t* __restrict__ perm, int64_t n,
               int n_aggs, BkKeyLayout kl, PostTypes pt, PostCols pc,
               uint32_t* nullmask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const int64_t g = live ? (perm ? (int64_t)perm[i] : i) : 0;
    uint32_t seen = 0;
    uint32_t flag = 0;
    uint64_t w0 = 0, w1 = 0;
    if (live && kl.n > 0) { flag = flags[g]; w0 = k0[g]; w1 = k1[g]; }

    /* group keys, decoded as AggNode::get_next does */
    #pragma unroll
    for (int k = 0; k < BK_MAX_GROUP; k++) {
        if (k < kl.n) {
            const bool has = !((flag >> (7 - k)) & 1);
            const int32_t ty = pt.key_type[k];
            const uint64_t out =
                bk_enc_to_cell(ty, bk_key_get(&kl, k, w0, w1, flag));
            if (post_store(pc.data[k], pc.valid[k], ty, i, live, has, out))
                seen |= 1u << k;
        }
    }

    #pragma unroll
    for (int a = 0; a < BK_MAX_AGGS; a++) {
        if (a < n_aggs) {
            uint64_t val = 0, cnt = 0;
            if (live) {
                const uint64_t* s = states + ((uint64_t)g * 2 * (uint64_t)n_aggs
                                              + 2 * (uint64_t)a);
                val = s[0];
                cnt = s[1];
            }
            uint64_t out;
            const bool has = bk_agg_finalize(pt.agg_type[a], pt.in_type[a],
                                             val, cnt, &out);
            if (post_store(pc.data[BK_MAX_GROUP + a], pc.valid[BK_MAX_GROUP + a],
                           bk_agg_out_type(pt.agg_type[a], pt.in_type[a]),
                           i, live, has, out))
                seen |= 1u << (BK_MAX_GROUP + a);
        }
    }
    if ((threadIdx.x & 63) == 0 && seen) atomicOr(nullmask, seen);
}

/* sort key of one canonical-order pass for output position i (group
 * perm[i], or i on the first pass): the key's packed field — order-
 * preserving within one key because every group shares the base — with
 * NULL keys as 0; nullbit < 0 selects the flag byte instead. */
__global__ void __launch_bounds__(256)
k_post_sortkey(const uint32_t* __restrict__ flags,
               const uint64_t* __restrict__ kw, const uint32_t* __restrict__ perm,
               int64_t n, int shift, uint64_t mask, int nullbit,
               uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = perm ? (int64_t)perm[i] : i;
    const uint32_t f = flags[g];
    if (nullbit < 0) { out[i] = f & 0xffu; return; }
    out[i] = ((f >> nullbit) & 1) ? 0 : ((kw[g] >> shift) & mask);
}

/* canonical MutTableKey order of the blob's groups as a device permutation
 * (the comparator of bkgpu_agg_fetch: flags first, then each non-NULL key's
 * encoding in key order): stable LSD radix passes from the last key to the
 * first, then the flag byte (pass p sorts key n_group - 1 - p; key -1 is the
 * flag byte). Returns the permutation, owned by bufs, or null. */
static uint32_t* post_canonical_perm(const BkgAggOut* o, PoolBufs& bufs) {
    const BkQuerySpec& q = o->q;
    const int64_t n = o->ngroups, c = o->blob_groups;
    const uint8_t* b = o->blob;
    const uint32_t* flags = (const uint32_t*)b;
    const uint64_t* kw[2] = {(const uint64_t*)(b + c * 4),
                             (const uint64_t*)(b + c * 12)};
    const BkKeyLayout kl = bk_key_layout(&q);
    const unsigned blocks = (unsigned)((n + 255) / 256);
    auto bits_of = [&](int pass) {
        const int k = q.n_group - 1 - pass;
        return k < 0 ? 8 : (int)kl.bits[k];
    };
    return dev_lsd_perm_sort(
        bufs, (uint64_t)n, q.n_group + 1, bits_of,
        [&](int pass, const uint32_t* perm, uint64_t* keys) {
            const int k = q.n_group - 1 - pass;
            const bool fl = k < 0;
            hipLaunchKernelGGL(k_post_sortkey, dim3(blocks), dim3(256), 0, 0,
                               flags, fl ? kw[0] : kw[kl.word[k]], perm, n,
                               fl ? 0 : kl.shift[k], bk_key_mask(bits_of(pass)),
                               fl ? -1 : 7 - k, keys);
        }, 256);
}

extern "C" BkgTable* bkgpu_agg_to_table(BkgAggOut* o, const BkgTable* dict_src,
                                        int canonical) {
    if (!o) { set_err("agg_to_table: null aggregate"); return nullptr; }
    if (ensure_device() != 0) return nullptr;
    if (agg_compact(o) != 0) return nullptr;
    const BkQuerySpec& q = o->q;
    const int64_t n = o->ngroups, c = o->blob_groups;
    if (n < 0 || n >= (int64_t(1) << 31)) {
        set_err("agg_to_table: group count out of range (>= 2^31)");
        return nullptr;
    }
    if (q.n_group < 0 || q.n_group > BK_MAX_GROUP || q.n_aggs < 0 ||
        q.n_aggs > BK_MAX_AGGS || q.n_group + q.n_aggs < 1) {
        set_err("agg_to_table: bad group/agg counts");
        return nullptr;
    }
    const bool timing = debug_timing();
    const BkKeyLayout kl = bk_key_layout(&q);
    PostTypes pt{};
    PostCols pc{};
    BkgTable* t = new BkgTable();
    t->ncols = q.n_group + q.n_aggs;
    t->nrows = n;
    int slot_of[POST_MAX_COLS];      /* table column -> PostCols slot */
    int src_col[POST_MAX_COLS];      /* dictionary source column, -1 none */
    for (int k = 0; k < q.n_group; k++) {
        pt.key_type[k] = q.group_fns[k] ? BK_INT64 : q.group_types[k];
        t->specs[k].col_type = pt.key_type[k];
        slot_of[k] = k;
        src_col[k] = q.group_cols[k];
    }
    for (int a = 0; a < q.n_aggs; a++) {
        const int at = q.aggs[a].agg_type, vt = q.agg_in_types[a];
        pt.agg_type[a] = at;
        pt.in_type[a] = vt;
        const int col = q.n_group + a;
        t->specs[col].col_type = bk_agg_out_type(at, vt);
        slot_of[col] = BK_MAX_GROUP + a;
        src_col[col] = ((at == BK_AGG_MIN || at == BK_AGG_MAX) &&
                        q.aggs[a].prog_len == 0) ? q.aggs[a].col : -1;
    }
    PoolBufs bufs;
    uint32_t* d_mask = nullptr;
    uint32_t* perm = nullptr;
    uint32_t h_mask = 0;
    double ms_sort = 0, ms_fin = 0;
    bool ok = true;
    for (int col = 0; ok && col < t->ncols; col++) {
        const bool count_shaped = col >= q.n_group &&
            bk_agg_count_shaped(pt.agg_type[col - q.n_group]);
        ok = table_alloc_col(t, col, t->specs[col].col_type, n,
                             !count_shaped && n > 0) == hipSuccess;
        if (!ok) set_err("agg_to_table: column allocation failed");
        pc.data[slot_of[col]] = t->data[col];
        pc.valid[slot_of[col]] = t->valid[col];
    }
    if (ok && n > 0) {
        if (canonical && q.n_group > 0 && n > 1) {
            double t0 = timing ? now_ms() : 0;
            perm = post_canonical_perm(o, bufs);
            ok = perm != nullptr;
            if (ok && timing) { (void)hipDeviceSynchronize(); ms_sort = now_ms() - t0; }
        }
        ok = ok && bufs.get(&d_mask, 4) == hipSuccess &&
             hipMemset(d_mask, 0, 4) == hipSuccess;
        if (ok) {
            const uint8_t* b = o->blob;
            double t0 = timing ? now_ms() : 0;
            hipLaunchKernelGGL(k_agg_finalize, dim3((unsigned)((n + 255) / 256)),
                               dim3(256), 0, 0,
                               (const uint32_t*)b, (const uint64_t*)(b + c * 4),
                               (const uint64_t*)(b + c * 12),
                               (const uint64_t*)(b + c * 20),
                               (const uint32_t*)perm, n, (int)q.n_aggs,
                               kl, pt, pc, d_mask);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpy(&h_mask, d_mask, 4, hipMemcpyDeviceToHost) == hipSuccess;
            if (!ok) set_err("agg_to_table: finalize kernel failed");
            if (timing) ms_fin = now_ms() - t0;
        }
    }
    if (!ok) { bkgpu_table_free(t); return nullptr; }
    for (int col = 0; col < t->ncols; col++)
        table_trim_validity(t, col, (h_mask >> slot_of[col]) & 1, dict_src,
                            src_col[col]);
    if (timing)
        fprintf(stderr, "[bkgpu] agg_to_table: %lld groups, perm sort %.3f ms, "
                        "finalize %.3f ms\n", (long long)n, ms_sort, ms_fin);
    return t;
}
