// bkjoin.inc — equi-join of two HBM tables into a table (bkgpu_join,
// include/bkgpu.h): the device form of JoinNode's hash join
// (src/exec/join_node.cpp, src/exec/joiner.cpp). Included from bkgpu.hip
// (shares BkgTable / DevCol / key_hash / k_dedup_mask; the host side is built
// from bkprim.inc — PoolBufs, BK_TRY, launch_grid, dev_*_scan,
// dev_lsd_perm_sort — and the table-column helpers next to
// bkgpu_table_create: table_alloc_col, table_trim_validity).
//
// Build side (inner): filter mask (k_dedup_mask) + key-non-NULL -> ordered
// compaction to (key words, inner row id) -> one stable rocPRIM radix pass
// per key column, last key first (equal keys end up adjacent with ascending
// row ids) -> head flags + scan -> runs (start, count) of unique keys -> the
// UNIQUE keys go into an open-addressing table (power-of-two slots, load
// <= 1/2). Every inserted key is distinct, so insertion never compares keys:
// a slot is claimed by one 32-bit CAS on its count word (0 = empty, a run
// count is never 0), the winner writes key words and run start with plain
// stores, and the kernel boundary publishes the table. No key value is
// reserved: emptiness lives in the count word, not in the key.
//
// Probe, two passes over fixed contiguous tiles of outer rows: k_join_count
// writes one u64 total per tile, a rocPRIM exclusive scan turns the totals
// into tile bases and the result size (the one host wait of the probe), and
// k_join_emit probes again, scans in row order inside the block and writes
// the pair list (outer row id, inner row id | NONE) at base + offset. No
// global cursor is touched per row (DESIGN.md §4). A lane loops over its own
// matches: one heavily duplicated key makes one lane's loop long (known
// limit, DESIGN.md §6).
//
// The join kernels take the key columns as individual by-value DevCol
// arguments and the side filter as the precomputed mask; they never call
// row_passes / eval_prog and never index a DevCols / BkQuerySpec kernarg with
// a runtime index (the kernarg-scratch trap, DESIGN.md §4/§6).

#define JOIN_BS 512                       /* threads per block */
#define JOIN_R 4                          /* outer rows per thread per tile */
#define JOIN_TILE (JOIN_BS * JOIN_R)      /* outer rows per tile */
#define JOIN_NW (JOIN_BS / 64)
#define JOIN_NONE 0xFFFFFFFFu             /* "no inner row" in the pair list */
#define JOIN_SCRATCH_WORDS 64             /* u64 scan scratch ahead of the LDS
                                           * slot copy (512 B, keeps the copy
                                           * 16-byte aligned) */
#define JOIN_LDS_CAP_KB 135
/* default of BK_JOIN_LDS_KB: slot arrays up to this many KB are probed from
 * LDS. Measured (DESIGN.md §4): the LDS route wins at 32 and 64 KB and
 * loses at 128 KB, where one block per CU is all that fits. */
#ifndef BK_JOIN_LDS_DEFAULT_KB
#define BK_JOIN_LDS_DEFAULT_KB 64
#endif

extern "C" int64_t bkgpu_join_tile_rows(void) { return JOIN_TILE; }

struct JoinStats {
    bool set = false;
    int64_t v[8] = {};
    double stage_ms[4] = {};
};
static thread_local JoinStats g_join_stats;

extern "C" int bkgpu_join_stats(int64_t out[8]) {
    if (!g_join_stats.set) { set_err("join_stats: no join on this thread"); return -1; }
    memcpy(out, g_join_stats.v, sizeof g_join_stats.v);
    return 0;
}
extern "C" int bkgpu_join_stage_ms(double out[4]) {
    if (!g_join_stats.set) { set_err("join_stats: no join on this thread"); return -1; }
    memcpy(out, g_join_stats.stage_ms, sizeof g_join_stats.stage_ms);
    return 0;
}

/* ---- keys ---- */
struct JoinKey { uint64_t w0, w1; bool ok; };

/* key words of row r (any row id inside the column); ok = no key is NULL.
 * NK == 1 leaves w1 = 0 and never touches k1. */
template <int NK>
__device__ __forceinline__ JoinKey join_key(const DevCol& k0, const DevCol& k1,
                                            int64_t r) {
    JoinKey k;
    k.ok = cell_valid(k0, r);
    k.w0 = (uint64_t)cell_i64(k0, r);
    k.w1 = 0;
    if (NK == 2) {
        k.ok = k.ok && cell_valid(k1, r);
        k.w1 = (uint64_t)cell_i64(k1, r);
    }
    return k;
}

__device__ __forceinline__ bool join_mask_bit(const uint64_t* mask, int64_t r) {
    return mask == nullptr || ((mask[(uint64_t)r >> 6] >> (r & 63)) & 1ull);
}

/* ---- build side ---- */

/* flag[i] = inner row i is a match candidate (passes the filter, no NULL
 * key); flag[n] = 0 so an exclusive scan over n + 1 entries also yields the
 * candidate count */
template <int NK>
__global__ void __launch_bounds__(256)
k_join_bflag(DevCol k0, DevCol k1, const uint64_t* __restrict__ mask, int64_t n,
             uint32_t* __restrict__ flag) {
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n;
         i += gs) {
        bool f = false;
        if (i < n && join_mask_bit(mask, i)) f = join_key<NK>(k0, k1, i).ok;
        flag[i] = f ? 1u : 0u;
    }
}

/* ordered compaction: candidate i lands at pos[i], so the compacted row ids
 * ascend with the index */
template <int NK>
__global__ void __launch_bounds__(256)
k_join_bcompact(DevCol k0, DevCol k1, const uint32_t* __restrict__ flag,
                const uint32_t* __restrict__ pos, int64_t n,
                uint64_t* __restrict__ ck0, uint64_t* __restrict__ ck1,
                uint32_t* __restrict__ crid) {
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        if (!flag[i]) continue;
        const JoinKey k = join_key<NK>(k0, k1, i);
        const uint32_t p = pos[i];
        ck0[p] = k.w0;
        if (NK == 2) ck1[p] = k.w1;
        crid[p] = (uint32_t)i;
    }
}

/* sort key of one radix pass: out[i] = ck[perm[i]] (perm == nullptr on the
 * first pass: identity) */
__global__ void __launch_bounds__(256)
k_join_permkey(const uint64_t* __restrict__ ck, const uint32_t* __restrict__ perm,
               uint64_t n, uint64_t* __restrict__ out) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        out[i] = ck[perm ? perm[i] : i];
}

/* after the sort: srid[i] = inner row id at sorted position i, head[i] = a
 * new key starts at i */
template <int NK>
__global__ void __launch_bounds__(256)
k_join_heads(const uint64_t* __restrict__ ck0, const uint64_t* __restrict__ ck1,
             const uint32_t* __restrict__ crid, const uint32_t* __restrict__ perm,
             uint64_t n, uint32_t* __restrict__ srid, uint32_t* __restrict__ head) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        const uint32_t p = perm[i];
        srid[i] = crid[p];
        bool h = true;
        if (i > 0) {
            const uint32_t pp = perm[i - 1];
            h = ck0[p] != ck0[pp];
            if (NK == 2) h = h || ck1[p] != ck1[pp];
        }
        head[i] = h ? 1u : 0u;
    }
}

/* ustart[u] = sorted position where unique key u starts (uidx = inclusive
 * scan of head, 1-based); ustart[nuniq] = n */
__global__ void __launch_bounds__(256)
k_join_runs(const uint32_t* __restrict__ head, const uint32_t* __restrict__ uidx,
            uint64_t n, uint32_t nuniq, uint32_t* __restrict__ ustart) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n;
         i += gs) {
        if (i == n) ustart[nuniq] = (uint32_t)n;
        else if (head[i]) ustart[uidx[i] - 1] = (uint32_t)i;
    }
}

/* slot = NK key words + one word {hi: run start, lo: run count}. The count
 * (>= 1 for a stored key) doubles as the claim word. */
template <int NK>
__global__ void __launch_bounds__(256)
k_join_insert(const uint64_t* __restrict__ ck0, const uint64_t* __restrict__ ck1,
              const uint32_t* __restrict__ perm, const uint32_t* __restrict__ ustart,
              uint32_t nuniq, uint64_t* slots, uint64_t smask) {
    constexpr int W = NK + 1;
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < nuniq;
         u += gs) {
        const uint32_t start = ustart[u], cnt = ustart[u + 1] - start;
        const uint32_t p = perm[start];
        const uint64_t w0 = ck0[p], w1 = NK == 2 ? ck1[p] : 0;
        uint64_t s = key_hash(0, w0, w1) & smask;
        /* load <= 1/2: an empty slot exists, the bound is a backstop */
        for (uint64_t probe = 0; probe <= smask; probe++) {
            uint64_t* sl = slots + s * W;
            uint32_t* meta = (uint32_t*)(sl + NK);      /* [0] count, [1] start */
            if (atomicCAS(meta, 0u, cnt) == 0u) {
                meta[1] = start;
                sl[0] = w0;
                if (NK == 2) sl[1] = w1;
                break;
            }
            s = (s + 1) & smask;
        }
    }
}

/* ---- probe ---- */

/* run (start, count) of key (w0, w1), count 0 = absent. `slots` is the HBM
 * array or the block's LDS copy of it; the caller picks with the
 * compile-time LDS flag, so after inlining the loads are global_ or ds_. */
template <int NK>
__device__ __forceinline__ uint32_t join_lookup(const uint64_t* slots,
                                                uint64_t smask, uint64_t w0,
                                                uint64_t w1, uint32_t* start) {
    constexpr int W = NK + 1;
    uint64_t s = key_hash(0, w0, w1) & smask;
    for (uint64_t probe = 0; probe <= smask; probe++) {
        const uint64_t* sl = slots + s * W;
        const uint64_t meta = sl[NK];
        const uint32_t cnt = (uint32_t)meta;
        if (cnt == 0) return 0;
        bool eq = sl[0] == w0;
        if (NK == 2) eq = eq && sl[1] == w1;
        if (eq) { *start = (uint32_t)(meta >> 32); return cnt; }
        s = (s + 1) & smask;
    }
    return 0;
}

/* stage the slot array for this block: the LDS route copies it behind the
 * scan scratch (every thread of the block must call this) */
template <bool LDS>
__device__ __forceinline__ const uint64_t* join_stage(uint64_t* jsm,
                                                      const uint64_t* gslots,
                                                      uint64_t nwords) {
    if (!LDS) return gslots;
    uint64_t* ltab = jsm + JOIN_SCRATCH_WORDS;
    for (uint64_t i = threadIdx.x; i < nwords; i += JOIN_BS) ltab[i] = gslots[i];
    __syncthreads();
    return ltab;
}

/* what one outer row emits: n output rows; cnt/start = its matching run */
struct JoinRow { uint32_t n, cnt, start; };

template <int NK>
__device__ __forceinline__ void join_tile_rows(
        const DevCol& k0, const DevCol& k1, const uint64_t* mask, int64_t nrows,
        int jt, const uint64_t* slots, uint64_t smask, int64_t tile,
        JoinRow (&row)[JOIN_R]) {
    /* keys first (clamped to a real row, so the loads batch), lookups after */
    JoinKey key[JOIN_R];
    bool pass[JOIN_R];
    #pragma unroll
    for (int j = 0; j < JOIN_R; j++) {
        const int64_t r = tile * JOIN_TILE + (int64_t)j * JOIN_BS + threadIdx.x;
        const int64_t rc = r < nrows ? r : nrows - 1;
        pass[j] = r < nrows && join_mask_bit(mask, rc);
        key[j] = join_key<NK>(k0, k1, rc);
    }
    #pragma unroll
    for (int j = 0; j < JOIN_R; j++) {
        uint32_t start = 0, cnt = 0;
        if (pass[j] && key[j].ok)
            cnt = join_lookup<NK>(slots, smask, key[j].w0, key[j].w1, &start);
        uint32_t n;
        if (jt == BK_INNER_JOIN) n = cnt;
        else if (jt == BK_LEFT_JOIN) n = cnt ? cnt : 1u;
        else if (jt == BK_SEMI_JOIN) n = cnt ? 1u : 0u;
        else n = cnt ? 0u : 1u;                         /* ANTI_SEMI */
        row[j].n = pass[j] ? n : 0u;
        row[j].cnt = cnt;
        row[j].start = start;
    }
}

/* pass 1: one u64 total per tile, nothing else */
template <int NK, bool LDS>
__global__ void __launch_bounds__(JOIN_BS)
k_join_count(DevCol k0, DevCol k1, const uint64_t* __restrict__ mask,
             int64_t nrows, int jt, const uint64_t* __restrict__ gslots,
             uint64_t nslots, int64_t ntiles, uint64_t* __restrict__ tile_tot) {
    extern __shared__ __attribute__((aligned(16))) uint64_t jsm[];
    const uint64_t* slots = join_stage<LDS>(jsm, gslots, nslots * (NK + 1));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        JoinRow row[JOIN_R];
        join_tile_rows<NK>(k0, k1, mask, nrows, jt, slots, nslots - 1, tile, row);
        uint64_t c = 0;
        #pragma unroll
        for (int j = 0; j < JOIN_R; j++) c += row[j].n;
        for (int off = 32; off > 0; off >>= 1)
            c += __shfl_down((unsigned long long)c, off, 64);
        if (lane == 0) jsm[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            #pragma unroll
            for (int w = 0; w < JOIN_NW; w++) t += jsm[w];
            tile_tot[tile] = t;
        }
        __syncthreads();                   /* jsm reused by the next tile */
    }
}

/* pass 2: probe again, exclusive scan in row order inside the block, write
 * the pairs at tile_base + offset. irid == nullptr for SEMI / ANTI. */
template <int NK, bool LDS>
__global__ void __launch_bounds__(JOIN_BS)
k_join_emit(DevCol k0, DevCol k1, const uint64_t* __restrict__ mask,
            int64_t nrows, int jt, const uint64_t* __restrict__ gslots,
            uint64_t nslots, int64_t ntiles,
            const uint64_t* __restrict__ tile_base,
            const uint32_t* __restrict__ srid, uint64_t total,
            uint32_t* __restrict__ orid, uint32_t* __restrict__ irid) {
    extern __shared__ __attribute__((aligned(16))) uint64_t jsm[];
    const uint64_t* slots = join_stage<LDS>(jsm, gslots, nslots * (NK + 1));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        JoinRow row[JOIN_R];
        join_tile_rows<NK>(k0, k1, mask, nrows, jt, slots, nslots - 1, tile, row);
        /* row order inside the tile is (j, thread): per j an inclusive wave
         * scan, wave totals to LDS, then the prefix over (j, wave) */
        uint64_t incl[JOIN_R];
        #pragma unroll
        for (int j = 0; j < JOIN_R; j++) {
            uint64_t v = row[j].n;
            #pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
                if (lane >= d) v += u;
            }
            incl[j] = v;
            if (lane == 63) jsm[j * JOIN_NW + wave] = v;
        }
        __syncthreads();
        uint64_t pre[JOIN_R] = {};
        uint64_t run = 0;
        #pragma unroll
        for (int j = 0; j < JOIN_R; j++) {
            #pragma unroll
            for (int w = 0; w < JOIN_NW; w++) {
                if (w == wave) pre[j] = run;
                run += jsm[j * JOIN_NW + w];
            }
        }
        const uint64_t base = tile_base[tile];
        #pragma unroll
        for (int j = 0; j < JOIN_R; j++) {
            if (row[j].n == 0) continue;
            const uint32_t r = (uint32_t)(tile * JOIN_TILE + (int64_t)j * JOIN_BS
                                          + threadIdx.x);
            const uint64_t o = base + pre[j] + incl[j] - row[j].n;
            if (o + row[j].n > total) continue;   /* cannot happen: both passes
                                                   * compute the same counts */
            if (irid == nullptr) {
                orid[o] = r;
            } else if (row[j].cnt == 0) {
                orid[o] = r;
                irid[o] = JOIN_NONE;
            } else {
                for (uint32_t m = 0; m < row[j].cnt; m++) {
                    orid[o + m] = r;
                    irid[o + m] = srid[row[j].start + m];
                }
            }
        }
        __syncthreads();                   /* jsm reused by the next tile */
    }
}

/* passing rows of a side = set bits of its mask */
__global__ void __launch_bounds__(256)
k_join_popc(const uint64_t* __restrict__ mask, uint64_t nwords,
            unsigned long long* out) {
    const uint64_t gs = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords;
         i += gs)
        c += (unsigned long long)__popcll(mask[i]);
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

/* materialize one output column: dst[o] = src[rid[o]] through the cell
 * accessor (8-byte cells; int32 codes for BK_STRING), coalesced writes.
 * rid == JOIN_NONE or a NULL source cell writes NULL. One ballot per wave
 * and one atomic record "this column saw a NULL" (k_agg_finalize pattern). */
__global__ void __launch_bounds__(256)
k_join_gather(DevCol c, const uint32_t* __restrict__ rid, int64_t n,
              void* __restrict__ dst, uint8_t* __restrict__ valid,
              uint32_t* nullmask, uint32_t bit) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    bool has = false;
    uint64_t v = 0;
    if (live) {
        const uint32_t r = rid[i];
        if (r != JOIN_NONE && cell_valid(c, (int64_t)r)) {
            has = true;
            v = (uint64_t)cell_i64(c, (int64_t)r);
        }
        if (c.type == BK_STRING) ((int32_t*)dst)[i] = (int32_t)(uint32_t)v;
        else ((uint64_t*)dst)[i] = v;
        if (valid) valid[i] = has ? 1 : 0;
    }
    const bool saw = __ballot(live && !has) != 0;
    if ((threadIdx.x & 63) == 0 && saw) atomicOr(nullmask, bit);
}

/* ---- host ---- */

/* side filter -> 1 bit per row (nullptr = every row passes) */
static int join_side_mask(BkgTable* t, const BkQuerySpec* q, PoolBufs& bufs,
                          uint64_t** mask, const char* side) {
    *mask = nullptr;
    if (!q || q->n_conjuncts == 0 || t->nrows == 0) return 0;
    if (q->n_conjuncts < 0 || q->n_conjuncts > BK_MAX_CONJUNCTS) {
        snprintf(g_err, sizeof g_err, "join: bad %s n_conjuncts", side);
        return -1;
    }
    for (int32_t j = 0; j < q->n_conjuncts; j++) {
        const BkConjunct& cj = q->conjuncts[j];
        if (cj.or_group < 0 || cj.or_group > 31 ||
            (cj.prog_len == 0 && (cj.col < 0 || cj.col >= t->ncols ||
                                  cj.col2 >= t->ncols))) {
            snprintf(g_err, sizeof g_err, "join: bad %s filter conjunct %d",
                     side, (int)j);
            return -1;
        }
    }
    if (query_exprs_check(t, q) != 0) return -1;
    const size_t words = ((size_t)t->nrows + 63) / 64;
    BK_TRY("join", bufs.get(mask, words * 8), -1);
    /* only the filter part of the spec reaches the mask kernel */
    BkQuerySpec qf = *q;
    qf.n_group = 0;
    qf.n_aggs = 0;
    hipLaunchKernelGGL(k_dedup_mask<false>, dim3(launch_grid(t->nrows, 512, 8192)),
                       dim3(512), 0, 0, table_cols(t), qf, (int64_t)0, t->nrows,
                       *mask);
    BK_TRY("join", hipGetLastError(), -1);
    return 0;
}

static int join_check_spec(const BkgTable* outer, const BkgTable* inner,
                           const BkJoinSpec* s) {
    if (!outer || !inner || !s) { set_err("join: null table or spec"); return -1; }
    const int jt = s->join_type;
    if (jt == BK_RIGHT_JOIN) {
        set_err("join: RIGHT_JOIN is not a kernel mode (swap the sides and "
                "run LEFT_JOIN)");
        return -1;
    }
    if (jt != BK_LEFT_JOIN && jt != BK_INNER_JOIN && jt != BK_SEMI_JOIN &&
        jt != BK_ANTI_SEMI_JOIN) {
        set_err("join: unsupported join type (FULL_JOIN / NULL_JOIN are not "
                "built)");
        return -1;
    }
    if (s->n_keys < 1 || s->n_keys > BK_MAX_JOIN_KEYS) {
        set_err("join: need 1 or 2 equality key pairs");
        return -1;
    }
    for (int k = 0; k < s->n_keys; k++) {
        const int oc = s->outer_key[k], ic = s->inner_key[k];
        if (oc < 0 || oc >= outer->ncols || ic < 0 || ic >= inner->ncols) {
            set_err("join: key column out of range");
            return -1;
        }
        const int ot = outer->specs[oc].col_type, it = inner->specs[ic].col_type;
        if (ot == BK_DOUBLE || it == BK_DOUBLE) {
            set_err("join: DOUBLE key columns are not supported");
            return -1;
        }
        if (ot == BK_STRING || it == BK_STRING) {
            set_err("join: STRING key columns are not supported (dict codes "
                    "of two tables are unrelated)");
            return -1;
        }
        if ((ot != BK_INT64 && ot != BK_DATETIME) || ot != it) {
            set_err("join: a key pair must be INT64/INT64 or "
                    "DATETIME/DATETIME");
            return -1;
        }
    }
    if (s->n_out < 1 || s->n_out > BK_MAX_COLS) {
        set_err("join: n_out must be 1..BK_MAX_COLS");
        return -1;
    }
    for (int c = 0; c < s->n_out; c++) {
        const int side = s->out_side[c], col = s->out_col[c];
        if (side != 0 && side != 1) { set_err("join: out_side must be 0 or 1"); return -1; }
        if (side == 1 && (jt == BK_SEMI_JOIN || jt == BK_ANTI_SEMI_JOIN)) {
            set_err("join: SEMI / ANTI_SEMI output takes outer-side columns only");
            return -1;
        }
        const BkgTable* src = side ? inner : outer;
        if (col < 0 || col >= src->ncols) { set_err("join: output column out of range"); return -1; }
    }
    if (outer->nrows >= (int64_t)JOIN_NONE || inner->nrows >= (int64_t)JOIN_NONE) {
        set_err("join: a side holds >= 2^32 - 1 rows (row ids are 32-bit)");
        return -1;
    }
    return 0;
}

template <int NK>
static BkgTable* join_run(BkgTable* outer, const BkQuerySpec* q_outer,
                          BkgTable* inner, const BkQuerySpec* q_inner,
                          const BkJoinSpec* s) {
    constexpr int W = NK + 1;
    const int jt = s->join_type;
    const bool pairs = jt == BK_INNER_JOIN || jt == BK_LEFT_JOIN;
    PoolBufs bufs;
    JoinStats st;
    const DevCols oc = table_cols(outer), ic = table_cols(inner);
    const DevCol ok0 = oc.c[s->outer_key[0]], ok1 = oc.c[s->outer_key[NK - 1]];
    const DevCol ik0 = ic.c[s->inner_key[0]], ik1 = ic.c[s->inner_key[NK - 1]];

    DevEvents<5> evs;
    hipEvent_t* ev = evs.e;
    BK_TRY("join", evs.create(), nullptr);
    (void)hipEventRecord(ev[0]);

    uint64_t *omask = nullptr, *imask = nullptr;
    if (join_side_mask(outer, q_outer, bufs, &omask, "outer") != 0) return nullptr;
    if (join_side_mask(inner, q_inner, bufs, &imask, "inner") != 0) return nullptr;

    /* ---- build ---- */
    const int64_t ni = inner->nrows;
    uint32_t *flag = nullptr, *pos = nullptr;
    BK_TRY("join", bufs.get(&flag, (size_t)(ni + 1) * 4), nullptr);
    BK_TRY("join", bufs.get(&pos, (size_t)(ni + 1) * 4), nullptr);
    hipLaunchKernelGGL(k_join_bflag<NK>, dim3(launch_grid(ni + 1)), dim3(256), 0, 0,
                       ik0, ik1, imask, ni, flag);
    BK_TRY("join", hipGetLastError(), nullptr);
    BK_TRY("join", dev_exclusive_scan(bufs, flag, pos, 0u, (size_t)(ni + 1),
                                      DevPlus<uint32_t>()), nullptr);
    uint32_t nb32 = 0;
    BK_TRY("join", hipMemcpy(&nb32, pos + ni, 4, hipMemcpyDeviceToHost), nullptr);
    const uint64_t nb = nb32;
    if (nb >= (1ull << 31)) {
        set_err("join: the inner side holds >= 2^31 passing rows");
        return nullptr;
    }
    uint64_t *ck0 = nullptr, *ck1 = nullptr;
    uint32_t *crid = nullptr, *perm = nullptr, *srid = nullptr, *ustart = nullptr;
    uint32_t nuniq = 0;
    if (nb > 0) {
        uint32_t *head = nullptr, *uidx = nullptr;
        BK_TRY("join", bufs.get(&ck0, nb * 8), nullptr);
        if (NK == 2) BK_TRY("join", bufs.get(&ck1, nb * 8), nullptr);
        BK_TRY("join", bufs.get(&crid, nb * 4), nullptr);
        BK_TRY("join", bufs.get(&srid, nb * 4), nullptr);
        BK_TRY("join", bufs.get(&head, nb * 4), nullptr);
        BK_TRY("join", bufs.get(&uidx, nb * 4), nullptr);
        hipLaunchKernelGGL(k_join_bcompact<NK>, dim3(launch_grid(ni)), dim3(256), 0,
                           0, ik0, ik1, flag, pos, ni, ck0, ck1, crid);
        BK_TRY("join", hipGetLastError(), nullptr);
        /* stable LSD passes, last key first: equal keys adjacent, compacted
         * indices (hence inner row ids) ascending inside a run */
        perm = dev_lsd_perm_sort(
            bufs, nb, NK, [](int) { return 64; },
            [&](int pass, const uint32_t* p, uint64_t* keys) {
                hipLaunchKernelGGL(k_join_permkey, dim3(launch_grid(nb)), dim3(256),
                                   0, 0, pass == NK - 1 ? ck0 : ck1, p, nb, keys);
            }, launch_grid(nb));
        if (!perm) return nullptr;
        hipLaunchKernelGGL(k_join_heads<NK>, dim3(launch_grid(nb)), dim3(256), 0, 0,
                           ck0, ck1, crid, perm, nb, srid, head);
        BK_TRY("join", hipGetLastError(), nullptr);
        BK_TRY("join", dev_inclusive_scan(bufs, head, uidx, (size_t)nb,
                                          DevPlus<uint32_t>()), nullptr);
        BK_TRY("join", hipMemcpy(&nuniq, uidx + (nb - 1), 4, hipMemcpyDeviceToHost),
               nullptr);
        BK_TRY("join", bufs.get(&ustart, ((size_t)nuniq + 1) * 4), nullptr);
        hipLaunchKernelGGL(k_join_runs, dim3(launch_grid(nb + 1)), dim3(256), 0, 0,
                           head, uidx, nb, nuniq, ustart);
        BK_TRY("join", hipGetLastError(), nullptr);
    }
    const uint64_t nslots = (uint64_t)std::max<int64_t>(16, next_pow2(2 * (int64_t)nuniq));
    const size_t slot_bytes = (size_t)nslots * W * 8;
    uint64_t* slots = nullptr;
    BK_TRY("join", bufs.get(&slots, slot_bytes), nullptr);
    BK_TRY("join", hipMemsetAsync(slots, 0, slot_bytes, 0), nullptr);
    if (nuniq > 0) {
        hipLaunchKernelGGL(k_join_insert<NK>, dim3(launch_grid(nuniq)), dim3(256), 0,
                           0, ck0, ck1, perm, ustart, nuniq, slots, nslots - 1);
        BK_TRY("join", hipGetLastError(), nullptr);
    }
    (void)hipEventRecord(ev[1]);

    /* ---- route: BK_JOIN_LDS_KB (0 = probe HBM/L2; else slot arrays up to
     * that many KB are copied into each block's LDS) ---- */
    int lds_kb = BK_JOIN_LDS_DEFAULT_KB;
    if (const char* e = getenv("BK_JOIN_LDS_KB")) lds_kb = atoi(e);
    lds_kb = std::max(0, std::min(lds_kb, JOIN_LDS_CAP_KB));
    const bool lds = lds_kb > 0 && slot_bytes <= (size_t)lds_kb * 1024;
    const size_t smem = JOIN_SCRATCH_WORDS * 8 + (lds ? slot_bytes : 0);

    /* ---- probe pass 1 ---- */
    const int64_t no = outer->nrows;
    const int64_t ntiles = (no + JOIN_TILE - 1) / JOIN_TILE;
    /* persistent blocks walk the tiles: the LDS route pays its slot copy
     * once per block; residency by LDS bytes (160 KB per CU, <= 4 blocks) */
    unsigned per_cu = 4;
    if (lds) per_cu = (unsigned)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / smem));
    const unsigned pgrid = (unsigned)std::max<int64_t>(
        1, std::min<int64_t>(ntiles, (int64_t)256 * per_cu));
    uint64_t *tile_tot = nullptr, *tile_base = nullptr;
    BK_TRY("join", bufs.get(&tile_tot, (size_t)(ntiles + 1) * 8), nullptr);
    BK_TRY("join", bufs.get(&tile_base, (size_t)(ntiles + 1) * 8), nullptr);
    BK_TRY("join", hipMemsetAsync(tile_tot + ntiles, 0, 8, 0), nullptr);
    auto count_fn = lds ? k_join_count<NK, true> : k_join_count<NK, false>;
    auto emit_fn = lds ? k_join_emit<NK, true> : k_join_emit<NK, false>;
    if (lds && smem > 64 * 1024) {
        (void)hipFuncSetAttribute((const void*)count_fn,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        (void)hipFuncSetAttribute((const void*)emit_fn,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    }
    if (ntiles > 0) {
        hipLaunchKernelGGL(count_fn, dim3(pgrid), dim3(JOIN_BS), smem, 0, ok0, ok1,
                           omask, no, jt, slots, nslots, ntiles, tile_tot);
        BK_TRY("join", hipGetLastError(), nullptr);
    }
    BK_TRY("join", dev_exclusive_scan(bufs, tile_tot, tile_base, (uint64_t)0,
                                      (size_t)(ntiles + 1), DevPlus<uint64_t>()),
           nullptr);
    /* passing outer rows, for the stats only */
    unsigned long long* d_pass = nullptr;
    BK_TRY("join", bufs.get(&d_pass, 8), nullptr);
    BK_TRY("join", hipMemsetAsync(d_pass, 0, 8, 0), nullptr);
    if (omask)
        hipLaunchKernelGGL(k_join_popc, dim3(launch_grid(((uint64_t)no + 63) / 64)),
                           dim3(256), 0, 0, omask, ((uint64_t)no + 63) / 64, d_pass);
    uint64_t total = 0;
    unsigned long long opass = 0;
    /* the one host wait of the probe: the result size */
    BK_TRY("join", hipMemcpy(&total, tile_base + ntiles, 8, hipMemcpyDeviceToHost),
           nullptr);
    BK_TRY("join", hipMemcpy(&opass, d_pass, 8, hipMemcpyDeviceToHost), nullptr);
    if (!omask) opass = (unsigned long long)no;
    (void)hipEventRecord(ev[2]);
    if (total >= (1ull << 31)) {
        snprintf(g_err, sizeof g_err,
                 "join: result of %llu rows exceeds the limit of 2^31 - 1 rows",
                 (unsigned long long)total);
        return nullptr;
    }

    /* ---- probe pass 2 ---- */
    const int64_t n = (int64_t)total;
    uint32_t *orid = nullptr, *irid = nullptr;
    BK_TRY("join", bufs.get(&orid, (size_t)n * 4), nullptr);
    if (pairs) BK_TRY("join", bufs.get(&irid, (size_t)n * 4), nullptr);
    if (n > 0) {
        hipLaunchKernelGGL(emit_fn, dim3(pgrid), dim3(JOIN_BS), smem, 0, ok0, ok1,
                           omask, no, jt, slots, nslots, ntiles, tile_base, srid,
                           total, orid, irid);
        BK_TRY("join", hipGetLastError(), nullptr);
    }
    (void)hipEventRecord(ev[3]);

    /* ---- materialize ---- */
    BkgTable* t = new BkgTable();
    t->ncols = s->n_out;
    t->nrows = n;
    uint32_t* d_null = nullptr;
    uint32_t h_null = 0;
    bool ok = bufs.get(&d_null, 4) == hipSuccess &&
              hipMemsetAsync(d_null, 0, 4, 0) == hipSuccess;
    if (!ok) set_err("join: null-mask allocation failed");
    for (int col = 0; ok && col < s->n_out; col++) {
        const bool in_side = s->out_side[col] == 1;
        const BkgTable* src = in_side ? inner : outer;
        const int sc = s->out_col[col];
        /* stored wide; a NULL can only come from a nullable source or a NULL
         * extension */
        const bool may_null = src->valid[sc] != nullptr ||
                              (in_side && jt == BK_LEFT_JOIN);
        ok = table_alloc_col(t, col, src->specs[sc].col_type, n,
                             may_null && n > 0) == hipSuccess;
        if (!ok) { set_err("join: hipMalloc of an output column failed"); break; }
        if (n > 0) {
            hipLaunchKernelGGL(k_join_gather, dim3((unsigned)((n + 255) / 256)),
                               dim3(256), 0, 0, (in_side ? ic : oc).c[sc],
                               in_side ? irid : orid, n, t->data[col],
                               t->valid[col], d_null, 1u << col);
            ok = hipGetLastError() == hipSuccess;
            if (!ok) set_err("join: gather kernel failed");
        }
    }
    if (ok) {
        ok = hipMemcpy(&h_null, d_null, 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (!ok) set_err("join: gather failed");
    }
    (void)hipEventRecord(ev[4]);
    if (!ok || hipEventSynchronize(ev[4]) != hipSuccess) {
        if (ok) set_err("join: device error");
        bkgpu_table_free(t);
        return nullptr;
    }
    for (int col = 0; col < s->n_out; col++)
        table_trim_validity(t, col, (h_null >> col) & 1,
                            s->out_side[col] ? inner : outer, s->out_col[col]);
    double tot_ms = 0;
    for (int i = 0; i < 4; i++) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
        st.stage_ms[i] = ms;
        tot_ms += ms;
    }
    st.v[0] = (int64_t)opass;
    st.v[1] = (int64_t)nb;
    st.v[2] = nuniq;
    st.v[3] = (int64_t)nslots;
    st.v[4] = n;
    st.v[5] = lds ? 1 : 0;
    st.v[6] = (int64_t)(tot_ms * 1000.0 + 0.5);
    st.v[7] = (int64_t)slot_bytes;
    st.set = true;
    g_join_stats = st;
    if (debug_timing())
        fprintf(stderr, "[bkgpu] join: %llu build rows, %u keys, %llu slots (%s), "
                        "%lld rows; build %.3f count %.3f emit %.3f gather %.3f ms\n",
                (unsigned long long)nb, nuniq, (unsigned long long)nslots,
                lds ? "lds" : "global", (long long)n, st.stage_ms[0],
                st.stage_ms[1], st.stage_ms[2], st.stage_ms[3]);
    return t;
}

extern "C" BkgTable* bkgpu_join(BkgTable* outer, const BkQuerySpec* q_outer,
                                BkgTable* inner, const BkQuerySpec* q_inner,
                                const BkJoinSpec* spec) {
    if (join_check_spec(outer, inner, spec) != 0) return nullptr;
    if (ensure_device() != 0) return nullptr;
    return spec->n_keys == 2
        ? join_run<2>(outer, q_outer, inner, q_inner, spec)
        : join_run<1>(outer, q_outer, inner, q_inner, spec);
}
