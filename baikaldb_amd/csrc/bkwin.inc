// bkwin.inc — WindowNode for gfx950, included into bkgpu.hip.
//
// Re-creates the reference's WindowNode + WindowFnCall in NON-FRAME mode
// (src/exec/window_node.cpp:39-41: no frame / UNBOUNDED-UNBOUNDED both run
// the NonFrameWindowProcessor — every fn sees its whole partition;
// src/expr/window_fn_call.cpp:364-700 call/get_result semantics).
//
// MI355X shape: the input is fully sorted by (partition, order keys,
// arrival) — the existing top-N selector with limit = all passing rows IS
// that sort (LSD radix over order-preserving encodings). Window evaluation
// is then three streaming passes over the sorted row ids:
//   1. k_win_flags : partition-change + peer-change flags (MemRowCompare
//      equality: NULLs compare equal, mem_row_compare.cpp:18-40)
//   2. rocprim scans: partition ids (sum), peer-group heads (max of
//      (partid<<40|pos), valid while n < 2^40 and np < 2^24 — the monotone
//      partition id in the high bits makes a global max-scan segment-local),
//      cumulative peer-change counts (dense rank)
//   3. k_win_agg : per-thread-slice segmented reduction of the aggregate
//      fns (atomic merges only at slice/partition boundaries — never
//      per-row, which would hit the ~20 G ops/s memory-side atomic wall)
//   4. k_win_emit: every fn's value per row from the scan arrays + the
//      per-partition states.

struct WinCompareCols {
    int32_t n_part;     /* 0 = single whole-set partition */
    int32_t part[3];    /* PARTITION BY columns (window_node.cpp evaluates
                           all partition exprs per row; a new partition
                           starts when ANY of them changes) */
    int32_t n_ord;
    int32_t ord[4];
};

/* value equality per MemRowCompare: NULLs equal each other */
__device__ __forceinline__ bool win_cell_eq(const DevCol& c, int64_t ra,
                                            int64_t rb) {
    bool va = cell_valid(c, ra), vb = cell_valid(c, rb);
    if (va != vb) return false;
    if (!va) return true;
    return enc_value(c, ra) == enc_value(c, rb);
}

__global__ void k_win_flags(DevCols cols, WinCompareCols w,
                            const int64_t* rowid, int64_t n,
                            uint32_t* segf, uint32_t* peerf) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        uint32_t s = 0, p = 0;
        if (i == 0) {
            s = p = 1;
        } else {
            for (int k = 0; k < w.n_part && !s; k++)
                if (!win_cell_eq(cols.c[w.part[k]], rowid[i], rowid[i - 1]))
                    s = 1;
            p = s;
            if (!p) {
                for (int k = 0; k < w.n_ord; k++) {
                    if (!win_cell_eq(cols.c[w.ord[k]], rowid[i], rowid[i - 1])) {
                        p = 1;
                        break;
                    }
                }
            }
        }
        segf[i] = s;
        peerf[i] = p;
    }
}

/* B[i] for the peer-head max-scan (see header comment) */
__global__ void k_win_peerpos(const uint32_t* partid1, const uint32_t* peerf,
                              int64_t n, uint64_t* B) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        B[i] = ((uint64_t)partid1[i] << 40) | (peerf[i] ? (uint64_t)i : 0);
}

/* partition bounds: part_start[partid1[i]-1] = i at each segment head */
/* per-peer-group end positions: peer groups are numbered globally by the
 * cumulative peer-change count (peerC); group g ends after max(i)+1 */
__global__ void k_win_peerend(const uint64_t* peerC, int64_t n,
                              uint64_t* peer_end) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        atomicMax((unsigned long long*)&peer_end[peerC[i]],
                  (unsigned long long)(i + 1));
}

__global__ void k_win_bounds(const uint32_t* partid1, const uint32_t* segf,
                             int64_t n, int64_t* bounds, int64_t np) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        if (segf[i]) bounds[partid1[i] - 1] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) bounds[np] = n;
}

/* per-partition aggregate states: [p][f] = {u64 val, u64 cnt}.
 * Each thread owns a CONTIGUOUS slice of rows and merges register
 * accumulators into the global state only when its run's partition ends. */
__global__ void k_win_agg(DevCols cols, WinCompareCols w, BkWindowFn fn0,
                          int nfns_dummy, const int64_t* rowid,
                          const uint32_t* partid1, int64_t n, int64_t rows_per,
                          uint64_t* states, const BkWindowFn* fns, int nfns) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t i0 = t * rows_per;
    if (i0 >= n) return;
    int64_t i1 = i0 + rows_per < n ? i0 + rows_per : n;
    (void)fn0; (void)nfns_dummy;
    /* scalarized accumulators for up to BK_MAX_WINFNS fns */
    uint64_t av[BK_MAX_WINFNS];
    uint64_t ac[BK_MAX_WINFNS];
    double ad[BK_MAX_WINFNS];
    uint32_t cur = partid1[i0];
    #pragma unroll
    for (int f = 0; f < BK_MAX_WINFNS; f++) { av[f] = 0; ac[f] = 0; ad[f] = 0; }
    auto flush = [&](uint32_t p1) {
        uint64_t* st = states + ((size_t)(p1 - 1) * nfns) * 2;
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            uint64_t* val = st + 2 * f;
            uint64_t* cnt = val + 1;
            switch (ft) {
                case BK_WIN_COUNT_STAR:
                case BK_WIN_COUNT:
                    if (ac[f]) atomicAdd((unsigned long long*)cnt,
                                         (unsigned long long)ac[f]);
                    break;
                case BK_WIN_SUM:
                case BK_WIN_AVG:
                    if (ac[f]) {
                        if (cols.c[fns[f].col].type == BK_DOUBLE ||
                            ft == BK_WIN_AVG)
                            atomic_add_f64_global(val, ad[f]);
                        else
                            atomicAdd((unsigned long long*)val,
                                      (unsigned long long)av[f]);
                        atomicAdd((unsigned long long*)cnt,
                                  (unsigned long long)ac[f]);
                    }
                    break;
                case BK_WIN_MIN:
                case BK_WIN_MAX:
                    if (ac[f]) {
                        atomicMax((unsigned long long*)val,
                                  (unsigned long long)av[f]);
                        atomicAdd((unsigned long long*)cnt,
                                  (unsigned long long)ac[f]);
                    }
                    break;
                default: break;
            }
        }
        for (int f = 0; f < nfns; f++) { av[f] = 0; ac[f] = 0; ad[f] = 0; }
    };
    for (int64_t i = i0; i < i1; i++) {
        uint32_t p1 = partid1[i];
        if (p1 != cur) { flush(cur); cur = p1; }
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            if (ft == BK_WIN_COUNT_STAR) { ac[f]++; continue; }
            if (ft > BK_WIN_MAX) continue;   /* rank/value fns: no state */
            const DevCol& c = cols.c[fns[f].col];
            if (!cell_valid(c, r)) continue;
            switch (ft) {
                case BK_WIN_COUNT: ac[f]++; break;
                case BK_WIN_SUM:
                    if (c.type == BK_DOUBLE) ad[f] += ((const double*)c.data)[r];
                    else av[f] += (uint64_t)cell_i64(c, r);
                    ac[f]++;
                    break;
                case BK_WIN_AVG: ad[f] += cell_f64(c, r); ac[f]++; break;
                case BK_WIN_MIN: {
                    uint64_t e = ~enc_value(c, r);
                    if (!ac[f] || e > av[f]) av[f] = e;
                    ac[f]++;
                    break;
                }
                case BK_WIN_MAX: {
                    uint64_t e = enc_value(c, r);
                    if (!ac[f] || e > av[f]) av[f] = e;
                    ac[f]++;
                    break;
                }
                default: break;
            }
        }
    }
    flush(cur);
}

/* ROWS-frame support (RowFrameWindowProcessor, window_node.cpp:49-58):
 * per frame-aggregate fn, GLOBAL inclusive prefix arrays over the sorted
 * stream — sum (u64 wrap for int64 inputs = reference modular adds; f64 for
 * double/avg) and non-null count. A frame [l,r] clamped inside the partition
 * then evaluates as prefix differences; partitions need no segmenting
 * because l,r never cross them. */
__global__ void k_win_frame_vals(DevCols cols, const int64_t* rowid,
                                 const BkWindowFn* fns, int nfns, int64_t n,
                                 uint64_t* S, uint64_t* Cc) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            int64_t idx = (int64_t)f * n + i;
            if (ft == BK_WIN_COUNT_STAR) { S[idx] = 0; Cc[idx] = 1; continue; }
            if (ft > BK_WIN_MAX || ft < BK_WIN_COUNT) { S[idx] = 0; Cc[idx] = 0; continue; }
            const DevCol& c = cols.c[fns[f].col];
            if (!cell_valid(c, r)) { S[idx] = 0; Cc[idx] = 0; continue; }
            Cc[idx] = 1;
            if (ft == BK_WIN_COUNT || ft == BK_WIN_MIN || ft == BK_WIN_MAX) {
                S[idx] = 0;
                continue;
            }
            if (c.type == BK_DOUBLE || ft == BK_WIN_AVG) {
                double d = cell_f64(c, r);
                memcpy(&S[idx], &d, 8);
            } else {
                S[idx] = (uint64_t)cell_i64(c, r);
            }
        }
    }
}

/* frame MIN/MAX: a sparse table over the order-encoded values of the
 * sorted stream (NULLs contribute the identity 0 — encodings of valid
 * values are handled as unsigned max; MIN uses the complement, exactly the
 * aggregate-state trick of DESIGN §2). Level k holds the max over
 * [i, i+2^k); a frame [l, r] is the max of two overlapping spans. Build is
 * log2(n) cheap passes; query O(1). */
__global__ void k_win_st_base(DevCols cols, const int64_t* rowid,
                              const BkWindowFn* fns, int nfns, int64_t n,
                              uint64_t* st /* [f][n] level 0 */) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        int64_t r = rowid[i];
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            if (ft != BK_WIN_MIN && ft != BK_WIN_MAX) continue;
            const DevCol& c = cols.c[fns[f].col];
            uint64_t e = 0;   /* NULL rows contribute the max-identity 0;
                                 emptiness is detected via the frame COUNT
                                 prefix (FC), not the value */
            if (cell_valid(c, r)) {
                e = enc_value(c, r);
                if (ft == BK_WIN_MIN) e = ~e;
            }
            st[(size_t)f * n + i] = e;
        }
    }
}

__global__ void k_win_st_level(const uint64_t* prev, uint64_t* cur,
                               int64_t n, int64_t span, int nfns) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    int64_t total = (int64_t)nfns * n;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total;
         x += gs) {
        int64_t i = x % n;
        int64_t j = i + span;
        uint64_t a = prev[x];
        if (j < n) {
            uint64_t b = prev[x - i + j];
            a = b > a ? b : a;
        }
        cur[x] = a;
    }
}

/* RANGE value-offset frames (mode 4): the order-key encodings of the
 * sorted stream, for per-row binary search of [v-pre, v+fol]. NULL-key
 * rows get 0 (they are excluded by the non-null span bounds). */
__global__ void k_win_ordenc(DevCols cols, int ord_col, const int64_t* rowid,
                             int64_t n, uint64_t* enc) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const DevCol& c = cols.c[ord_col];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs)
        enc[i] = cell_valid(c, rowid[i]) ? enc_value(c, rowid[i]) : 0;
}

/* one output value: loads input col at sorted position j (global row
 * rowid[j]); writes typed out + null flag */
__device__ __forceinline__ void win_emit_value(const DevCols& cols, int col,
                                               const int64_t* rowid, int64_t j,
                                               int64_t idx, int64_t* out_i,
                                               double* out_d, uint8_t* out_null) {
    const DevCol& c = cols.c[col];
    int64_t r = rowid[j];
    if (!cell_valid(c, r)) { out_null[idx] = 1; return; }
    out_null[idx] = 0;
    if (c.type == BK_DOUBLE) out_d[idx] = ((const double*)c.data)[r];
    else out_i[idx] = cell_i64(c, r);
}

__global__ void k_win_emit(DevCols cols, const int64_t* rowid,
                           const uint32_t* partid1, const uint64_t* peerB,
                           const uint64_t* peerC, const uint64_t* peer_end,
                           const int64_t* bounds,
                           const uint64_t* states, const BkWindowFn* fns,
                           int nfns, int64_t n, int frame_rows, int64_t f_pre,
                           int64_t f_fol, const uint64_t* FS,
                           const uint64_t* FC, const uint64_t* ST, int st_levels,
                           const uint64_t* ENCo, int ord_col,
                           int ord_null_first,
                           int64_t* out_i, double* out_d, uint8_t* out_null) {
    int64_t gs = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gs) {
        uint32_t p1 = partid1[i];
        int64_t ps = bounds[p1 - 1], pe = bounds[p1];
        int64_t pn = pe - ps;
        int64_t peer_head = (int64_t)(peerB[i] & 0xFFFFFFFFFFull);
        const uint64_t* st = states + ((size_t)(p1 - 1) * nfns) * 2;
        /* frame bounds for this row (clamped to the partition).
         * mode 1: ROWS [i-f_pre, i+f_fol]; mode 2: RANGE UNBOUNDED
         * PRECEDING..CURRENT ROW = [ps, end of current peer group); mode 3:
         * RANGE CURRENT ROW..UNBOUNDED FOLLOWING = [peer head, pe). */
        int64_t fl = ps, fr = pe - 1;
        if (frame_rows == 1) {
            if (f_pre >= 0) fl = i - f_pre > ps ? i - f_pre : ps;
            if (f_fol >= 0) fr = i + f_fol < pe - 1 ? i + f_fol : pe - 1;
        } else if (frame_rows == 2) {
            fr = (int64_t)peer_end[peerC[i]] - 1;
        } else if (frame_rows == 3) {
            fl = peer_head;
        } else if (frame_rows == 4) {
            /* RANGE BETWEEN f_pre PRECEDING AND f_fol FOLLOWING by VALUE
             * over the single ASC integer order key (negative bound =
             * UNBOUNDED). NULL-key rows frame their own peer group (NULLs
             * are peers); non-null rows binary-search the partition's
             * non-null span over the order-key encodings. */
            const DevCol& oc = cols.c[ord_col];
            if (oc.valid && !cell_valid(oc, rowid[i])) {
                fl = peer_head;
                fr = (int64_t)peer_end[peerC[i]] - 1;
            } else {
                int64_t nn_lo = ps, nn_hi = pe;
                if (oc.valid) {
                    if (ord_null_first) {
                        if (!cell_valid(oc, rowid[ps]))
                            nn_lo = (int64_t)peer_end[peerC[ps]];
                    } else {
                        if (!cell_valid(oc, rowid[pe - 1]))
                            nn_hi = (int64_t)(peerB[pe - 1] & 0xFFFFFFFFFFull);
                    }
                }
                uint64_t v = ENCo[i];
                if (f_pre < 0) {
                    fl = nn_lo;
                } else {
                    uint64_t lo_t = v >= (uint64_t)f_pre ? v - (uint64_t)f_pre
                                                         : 0;
                    int64_t lo = nn_lo, hi = i;
                    while (lo < hi) {
                        int64_t mid = (lo + hi) >> 1;
                        if (ENCo[mid] < lo_t) lo = mid + 1; else hi = mid;
                    }
                    fl = lo;
                }
                if (f_fol < 0) {
                    fr = nn_hi - 1;
                } else {
                    uint64_t hi_t = v + (uint64_t)f_fol >= v
                                        ? v + (uint64_t)f_fol : ~0ull;
                    int64_t lo = i, hi = nn_hi;
                    while (lo < hi) {
                        int64_t mid = (lo + hi) >> 1;
                        if (ENCo[mid] <= hi_t) lo = mid + 1; else hi = mid;
                    }
                    fr = lo - 1;
                }
            }
        }
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            int64_t idx = (int64_t)f * n + i;
            uint64_t val = st[2 * f], cnt = st[2 * f + 1];
            out_i[idx] = 0; out_d[idx] = 0.0; out_null[idx] = 0;
            if (frame_rows && (ft == BK_WIN_MIN || ft == BK_WIN_MAX)) {
                if (fr < fl) { out_null[idx] = 1; continue; }
                const uint64_t* Cf = FC + (size_t)f * n;
                uint64_t fcnt = Cf[fr] - (fl > 0 ? Cf[fl - 1] : 0);
                if (!fcnt) { out_null[idx] = 1; continue; }  /* all NULL */
                int64_t len = fr - fl + 1;
                int k = 63 - __clzll((unsigned long long)len);
                if (k >= st_levels) k = st_levels - 1;
                const uint64_t* Lk = ST + ((size_t)k * nfns + f) * n;
                uint64_t a = Lk[fl];
                uint64_t b = Lk[fr - (1ll << k) + 1];
                uint64_t e = a > b ? a : b;
                if (ft == BK_WIN_MIN) e = ~e;
                const DevCol& c = cols.c[fns[f].col];
                if (c.type == BK_DOUBLE) out_d[idx] = bk_dec_f64(e);
                else if (c.type == BK_STRING) out_i[idx] = (int64_t)(uint32_t)e;
                else out_i[idx] = bk_dec_i64(e);
                continue;
            }
            if (frame_rows && ft <= BK_WIN_AVG) {
                /* frame aggregates from the prefix arrays */
                const uint64_t* Sf = FS + (size_t)f * n;
                const uint64_t* Cf = FC + (size_t)f * n;
                if (fr < fl) {   /* empty frame */
                    if (ft == BK_WIN_COUNT_STAR || ft == BK_WIN_COUNT)
                        out_i[idx] = 0;
                    else out_null[idx] = 1;
                    continue;
                }
                uint64_t fcnt = Cf[fr] - (fl > 0 ? Cf[fl - 1] : 0);
                if (ft == BK_WIN_COUNT_STAR || ft == BK_WIN_COUNT) {
                    out_i[idx] = (int64_t)fcnt;
                    continue;
                }
                if (!fcnt) { out_null[idx] = 1; continue; }
                if (cols.c[fns[f].col].type == BK_DOUBLE || ft == BK_WIN_AVG) {
                    double sum;
                    if (fr - fl < 64) {
                        /* SHORT frames sum directly in frame order — the
                         * reference accumulates per frame (ExprValue::add
                         * sequence), so its error is ~ulp(frame sum); a
                         * prefix DIFFERENCE carries ~ulp(prefix total),
                         * which at 2^40-scale int64 inputs over 2e4 rows
                         * exceeds the documented 1e-10 tolerance (observed
                         * |err| 2.5 on a 2-row AVG frame). */
                        const DevCol& c = cols.c[fns[f].col];
                        sum = 0.0;
                        for (int64_t j = fl; j <= fr; j++) {
                            int64_t r = rowid[j];
                            if (cell_valid(c, r)) sum += cell_f64(c, r);
                        }
                    } else {
                        double hi, lo = 0.0;
                        memcpy(&hi, &Sf[fr], 8);
                        if (fl > 0) memcpy(&lo, &Sf[fl - 1], 8);
                        sum = hi - lo;
                    }
                    out_d[idx] = ft == BK_WIN_AVG ? sum / (double)fcnt : sum;
                } else {
                    out_i[idx] = (int64_t)(Sf[fr] - (fl > 0 ? Sf[fl - 1] : 0));
                }
                continue;
            }
            switch (ft) {
                case BK_WIN_COUNT_STAR:
                case BK_WIN_COUNT: out_i[idx] = (int64_t)cnt; break;
                case BK_WIN_SUM:
                    if (!cnt) { out_null[idx] = 1; break; }
                    if (cols.c[fns[f].col].type == BK_DOUBLE) {
                        double d; memcpy(&d, &val, 8); out_d[idx] = d;
                    } else out_i[idx] = (int64_t)val;
                    break;
                case BK_WIN_AVG:
                    if (!cnt) { out_null[idx] = 1; break; }
                    { double d; memcpy(&d, &val, 8); out_d[idx] = d / (double)cnt; }
                    break;
                case BK_WIN_MIN:
                case BK_WIN_MAX: {
                    if (!cnt) { out_null[idx] = 1; break; }
                    uint64_t e = ft == BK_WIN_MIN ? ~val : val;
                    const DevCol& c = cols.c[fns[f].col];
                    if (c.type == BK_DOUBLE) out_d[idx] = bk_dec_f64(e);
                    else if (c.type == BK_STRING) out_i[idx] = (int64_t)(uint32_t)e;
                    else out_i[idx] = bk_dec_i64(e);
                    break;
                }
                case BK_WIN_ROW_NUMBER: out_i[idx] = i - ps + 1; break;
                case BK_WIN_RANK: out_i[idx] = peer_head - ps + 1; break;
                case BK_WIN_DENSE_RANK:
                    out_i[idx] = (int64_t)(peerC[i] - peerC[ps]) + 1;
                    break;
                case BK_WIN_PERCENT_RANK:
                    /* (rank-1)/(n-1); 0 for single-row partitions
                     * (window_fn_call.cpp:570-607) */
                    out_d[idx] = pn > 1
                        ? (double)(peer_head - ps) / (double)(pn - 1) : 0.0;
                    break;
                case BK_WIN_FIRST_VALUE:
                    if (fr < fl) { out_null[idx] = 1; break; }
                    win_emit_value(cols, fns[f].col, rowid, fl, idx,
                                   out_i, out_d, out_null);
                    break;
                case BK_WIN_LAST_VALUE:
                    if (fr < fl) { out_null[idx] = 1; break; }
                    win_emit_value(cols, fns[f].col, rowid, fr, idx,
                                   out_i, out_d, out_null);
                    break;
                case BK_WIN_NTH_VALUE: {
                    int64_t j = fl + fns[f].param - 1;
                    if (j >= fl && j <= fr)
                        win_emit_value(cols, fns[f].col, rowid, j, idx,
                                       out_i, out_d, out_null);
                    else out_null[idx] = 1;
                    break;
                }
                case BK_WIN_LEAD:
                case BK_WIN_LAG: {
                    int64_t off = fns[f].param > 0 ? fns[f].param : 1;
                    int64_t j = ft == BK_WIN_LEAD ? i + off : i - off;
                    if (j >= ps && j < pe) {
                        win_emit_value(cols, fns[f].col, rowid, j, idx,
                                       out_i, out_d, out_null);
                    } else if (fns[f].has_def) {
                        if (cols.c[fns[f].col].type == BK_DOUBLE)
                            out_d[idx] = fns[f].def_d;
                        else out_i[idx] = fns[f].def_i;
                    } else {
                        out_null[idx] = 1;
                    }
                    break;
                }
                case BK_WIN_CUME_DIST:
                    /* rows <= current peer group / partition rows
                     * (window_fn_call.cpp:609-655) */
                    out_d[idx] = (double)((int64_t)peer_end[peerC[i]] - ps) /
                                 (double)pn;
                    break;
                case BK_WIN_NTILE: {
                    /* first `rem` buckets take quot+1 rows
                     * (window_fn_call.cpp:456-467, NTILE get_result) */
                    int64_t k = fns[f].param > 0 ? fns[f].param : 1;
                    int64_t quot = pn / k, rem = pn % k;
                    int64_t j = i - ps;
                    int64_t fat = rem * (quot + 1);
                    out_i[idx] = j < fat
                        ? j / (quot + 1) + 1
                        : rem + (quot > 0 ? (j - fat) / quot : 0) + 1;
                    break;
                }
                default: out_null[idx] = 1; break;
            }
        }
    }
}

/* host: the full window pipeline. Returns rows produced (= rows passing q),
 * <0 on error. Outputs fn-major: out_i/out_d/out_null[f*n + i], rows in
 * (partition, order, arrival) order with their global ids in out_rowids. */
/* frame_rows == 0: non-frame (whole partition). 1: ROWS BETWEEN f_pre
 * PRECEDING AND f_fol FOLLOWING (negative bound = UNBOUNDED; 0 = CURRENT
 * ROW). 2: RANGE UNBOUNDED PRECEDING..CURRENT ROW (running totals with
 * ties — the frame ends at the current PEER GROUP's end). 3: RANGE CURRENT
 * ROW..UNBOUNDED FOLLOWING. 4: RANGE BETWEEN f_pre PRECEDING AND f_fol
 * FOLLOWING by VALUE (single ASC integer order key; NULL-key rows frame
 * their peer group). All frame modes support SUM/COUNT/COUNT(*)/AVG/MIN/
 * MAX and FIRST/LAST/NTH_VALUE
 * (RowFrame/RangeFrameWindowProcessor, window_node.cpp:49-58). */
extern "C" int64_t bkgpu_window_multi(BkgTable* t, const BkQuerySpec* q,
                                const int32_t* part_cols, int32_t n_part,
                                const BkOrderSpec* order, int norder,
                                const BkWindowFn* fns, int nfns,
                                int32_t frame_rows, int64_t f_pre, int64_t f_fol,
                                int64_t row_begin, int64_t row_end,
                                int64_t* out_rowids, int64_t* out_i,
                                double* out_d, uint8_t* out_null) {
    if (nfns < 1 || nfns > BK_MAX_WINFNS) { set_err("window: bad nfns"); return -1; }
    if (norder < 0 || norder > 3) { set_err("window: bad norder"); return -1; }
    if (n_part < 0 || n_part > 3) { set_err("window: bad n_part"); return -1; }
    if (n_part + norder > 4) {
        set_err("window: n_part + norder > 4 sort keys");
        return -1;
    }
    for (int k = 0; k < n_part; k++)
        if (part_cols[k] < 0 || part_cols[k] >= t->ncols) {
            set_err("window: bad partition col");
            return -1;
        }
    bool frame_minmax = false;
    if (frame_rows)
        for (int f = 0; f < nfns; f++)
            frame_minmax |= fns[f].fn_type == BK_WIN_MIN ||
                            fns[f].fn_type == BK_WIN_MAX;
    if (frame_rows == 4) {
        int oc = norder == 1 ? order[0].col : -1;
        int32_t octy = oc >= 0 ? t->specs[oc].col_type : -1;
        if (norder != 1 || !order[0].is_asc ||
            (octy != BK_INT64 && octy != BK_DATETIME)) {
            set_err("window: RANGE value frames need one ASC integer "
                    "order key");
            return -1;
        }
    }
    for (int f = 0; f < nfns; f++) {
        int ft = fns[f].fn_type;
        bool needs_col = !(ft == BK_WIN_COUNT_STAR || ft == BK_WIN_ROW_NUMBER ||
                           ft == BK_WIN_RANK || ft == BK_WIN_DENSE_RANK ||
                           ft == BK_WIN_PERCENT_RANK || ft == BK_WIN_CUME_DIST ||
                           ft == BK_WIN_NTILE);
        if (needs_col && (fns[f].col < 0 || fns[f].col >= t->ncols)) {
            set_err("window: bad fn col");
            return -1;
        }
    }
    /* 1. full sort by (partition, order, arrival) via the top-N machinery
     * with limit = everything */
    BkOrderSpec full[4];
    int nf = 0;
    for (int k = 0; k < n_part; k++) full[nf++] = {part_cols[k], 1, 1, 0};
    for (int k = 0; k < norder && nf < 4; k++) full[nf++] = order[k];
    int64_t range = row_end - row_begin;
    int64_t n;
    if (nf == 0) {
        /* no partition, no order keys: output order = arrival order */
        n = bkgpu_filter_collect(t, q, row_begin, row_end, range, out_rowids);
        if (n > 0) std::sort(out_rowids, out_rowids + n);
    } else {
        n = bkgpu_sort_topk(t, q, full, nf, row_begin, row_end, range,
                            out_rowids);
    }
    if (n < 0) return n;
    if (n == 0) return 0;
    if (n >= (1ll << 40)) { set_err("window: too many rows"); return -1; }

    int64_t* rowid = nullptr;
    uint32_t *segf = nullptr, *peerf = nullptr, *partid1 = nullptr;
    uint64_t *peerB = nullptr, *peerC = nullptr, *states = nullptr;
    uint64_t *peer_end = nullptr, *FS = nullptr, *FC = nullptr;
    uint64_t *ST = nullptr, *ENCo = nullptr;
    int st_levels = 0;
    int64_t* bounds = nullptr;
    BkWindowFn* dfns = nullptr;
    int64_t* d_out_i = nullptr;
    double* d_out_d = nullptr;
    uint8_t* d_out_null = nullptr;
    PoolBufs bufs;
    BK_TRY("window", bufs.get(&rowid, (size_t)n * 8), -1);
    BK_TRY("window", hipMemcpy(rowid, out_rowids, (size_t)n * 8,
                               hipMemcpyHostToDevice), -1);
    BK_TRY("window", bufs.get(&segf, (size_t)n * 4), -1);
    BK_TRY("window", bufs.get(&peerf, (size_t)n * 4), -1);
    BK_TRY("window", bufs.get(&partid1, (size_t)n * 4), -1);
    BK_TRY("window", bufs.get(&peerB, (size_t)n * 8), -1);
    BK_TRY("window", bufs.get(&peerC, (size_t)n * 8), -1);
    BK_TRY("window", bufs.get(&dfns, sizeof(BkWindowFn) * (size_t)nfns), -1);
    BK_TRY("window", hipMemcpy(dfns, fns, sizeof(BkWindowFn) * (size_t)nfns,
                               hipMemcpyHostToDevice), -1);

    DevCols dc = table_cols(t);
    WinCompareCols w{};
    w.n_part = n_part;
    for (int k = 0; k < n_part; k++) w.part[k] = part_cols[k];
    w.n_ord = norder;
    for (int k = 0; k < norder; k++) w.ord[k] = order[k].col;
    int blocks = 2048, threads = 256;
    hipLaunchKernelGGL(k_win_flags, dim3(blocks), dim3(threads), 0, 0,
                       dc, w, rowid, n, segf, peerf);
    /* partition ids (1-based): inclusive sum scan of segf */
    BK_TRY("window", dev_inclusive_scan(bufs, segf, partid1, (size_t)n,
                                        DevPlus<uint32_t>()), -1);
    BK_TRY("window", dev_inclusive_scan(bufs, peerf, peerC, (size_t)n,
                                        DevPlus<uint64_t>()), -1);
    hipLaunchKernelGGL(k_win_peerpos, dim3(blocks), dim3(threads), 0, 0,
                       partid1, peerf, n, peerB);
    BK_TRY("window", dev_inclusive_scan(bufs, peerB, peerB, (size_t)n,
                                        DevMax<uint64_t>()), -1);
    uint32_t np = 0;
    BK_TRY("window", hipMemcpy(&np, partid1 + (n - 1), 4, hipMemcpyDeviceToHost), -1);
    if (np >= (1u << 24)) { set_err("window: too many partitions"); return -1; }
    BK_TRY("window", bufs.get(&bounds, ((size_t)np + 1) * 8), -1);
    hipLaunchKernelGGL(k_win_bounds, dim3(blocks), dim3(threads), 0, 0,
                       partid1, segf, n, bounds, (int64_t)np);
    BK_TRY("window", bufs.get(&states, (size_t)np * nfns * 2 * 8), -1);
    BK_TRY("window", hipMemset(states, 0, (size_t)np * nfns * 2 * 8), -1);
    bool any_agg = false;
    for (int f = 0; f < nfns; f++) any_agg |= fns[f].fn_type <= BK_WIN_MAX;
    if (any_agg) {
        int64_t total_threads = (int64_t)blocks * threads;
        int64_t rows_per = (n + total_threads - 1) / total_threads;
        hipLaunchKernelGGL(k_win_agg, dim3(blocks), dim3(threads), 0, 0,
                           dc, w, fns[0], nfns, rowid, partid1, n, rows_per,
                           states, dfns, nfns);
    }
    uint64_t total_peers = 0;
    BK_TRY("window", hipMemcpy(&total_peers, peerC + (n - 1), 8,
                               hipMemcpyDeviceToHost), -1);
    BK_TRY("window", bufs.get(&peer_end, (total_peers + 1) * 8), -1);
    BK_TRY("window", hipMemset(peer_end, 0, (total_peers + 1) * 8), -1);
    hipLaunchKernelGGL(k_win_peerend, dim3(blocks), dim3(threads), 0, 0,
                       peerC, n, peer_end);
    if (frame_rows) {
        BK_TRY("window", bufs.get(&FS, (size_t)nfns * n * 8), -1);
        BK_TRY("window", bufs.get(&FC, (size_t)nfns * n * 8), -1);
        hipLaunchKernelGGL(k_win_frame_vals, dim3(blocks), dim3(threads), 0, 0,
                           dc, rowid, dfns, nfns, n, FS, FC);
        for (int f = 0; f < nfns; f++) {
            int ft = fns[f].fn_type;
            if (ft > BK_WIN_MAX) continue;
            uint64_t* Sf = FS + (size_t)f * n;
            uint64_t* Cf = FC + (size_t)f * n;
            BK_TRY("window", dev_inclusive_scan(bufs, Cf, Cf, (size_t)n,
                                                DevPlus<uint64_t>()), -1);
            if (ft == BK_WIN_MIN || ft == BK_WIN_MAX || ft == BK_WIN_COUNT ||
                ft == BK_WIN_COUNT_STAR)
                continue;   /* counts only */
            bool dbl = fns[f].fn_type == BK_WIN_AVG ||
                       (fns[f].col >= 0 &&
                        t->specs[fns[f].col].col_type == BK_DOUBLE);
            if (dbl)
                BK_TRY("window", dev_inclusive_scan(bufs, (double*)Sf, (double*)Sf,
                                                    (size_t)n, DevPlus<double>()), -1);
            else
                BK_TRY("window", dev_inclusive_scan(bufs, Sf, Sf, (size_t)n,
                                                    DevPlus<uint64_t>()), -1);
        }
    }
    /* sparse table for frame MIN/MAX: levels sized by the max frame length
     * (bounded ROWS frames need only log2(pre+fol+1)+1 levels) */
    if (frame_rows && frame_minmax) {
        int64_t maxlen = n;
        if (frame_rows == 1 && f_pre >= 0 && f_fol >= 0)
            maxlen = f_pre + f_fol + 1;
        if (maxlen > n) maxlen = n;
        st_levels = 1;
        while ((1ll << st_levels) < maxlen && st_levels < 40) st_levels++;
        st_levels += (1ll << (st_levels - 1)) < maxlen ? 1 : 0;
        if (st_levels < 1) st_levels = 1;
        size_t st_bytes = (size_t)st_levels * nfns * (size_t)n * 8;
        if (st_bytes > (size_t)8 << 30) {
            set_err("window: frame MIN/MAX sparse table would exceed 8 GB "
                    "(bound the frame or reduce rows)");
            return -1;
        }
        BK_TRY("window", bufs.get(&ST, st_bytes), -1);
        hipLaunchKernelGGL(k_win_st_base, dim3(blocks), dim3(threads), 0, 0,
                           dc, rowid, dfns, nfns, n, ST);
        for (int k = 1; k < st_levels; k++) {
            hipLaunchKernelGGL(k_win_st_level, dim3(blocks), dim3(threads),
                               0, 0, ST + ((size_t)(k - 1) * nfns) * n,
                               ST + ((size_t)k * nfns) * n, n,
                               (int64_t)1 << (k - 1), nfns);
        }
    }
    int ord_col = norder >= 1 ? order[0].col : -1;
    int ord_nf = norder >= 1 ? order[0].is_null_first : 1;
    if (frame_rows == 4) {
        BK_TRY("window", bufs.get(&ENCo, (size_t)n * 8), -1);
        hipLaunchKernelGGL(k_win_ordenc, dim3(blocks), dim3(threads), 0, 0,
                           dc, ord_col, rowid, n, ENCo);
    }
    BK_TRY("window", bufs.get(&d_out_i, (size_t)nfns * n * 8), -1);
    BK_TRY("window", bufs.get(&d_out_d, (size_t)nfns * n * 8), -1);
    BK_TRY("window", bufs.get(&d_out_null, (size_t)nfns * n), -1);
    hipLaunchKernelGGL(k_win_emit, dim3(blocks), dim3(threads), 0, 0,
                       dc, rowid, partid1, peerB, peerC, peer_end, bounds,
                       states, dfns, nfns, n, frame_rows, f_pre, f_fol,
                       FS, FC, ST, st_levels, ENCo, ord_col, ord_nf,
                       d_out_i, d_out_d, d_out_null);
    BK_TRY("window", hipGetLastError(), -1);
    BK_TRY("window", hipMemcpy(out_i, d_out_i, (size_t)nfns * n * 8,
                               hipMemcpyDeviceToHost), -1);
    BK_TRY("window", hipMemcpy(out_d, d_out_d, (size_t)nfns * n * 8,
                               hipMemcpyDeviceToHost), -1);
    BK_TRY("window", hipMemcpy(out_null, d_out_null, (size_t)nfns * n,
                               hipMemcpyDeviceToHost), -1);
    return n;
}

/* single-partition-column compatibility entry (the round-1 surface) */
extern "C" int64_t bkgpu_window(BkgTable* t, const BkQuerySpec* q,
                                int32_t part_col,
                                const BkOrderSpec* order, int norder,
                                const BkWindowFn* fns, int nfns,
                                int32_t frame_rows, int64_t f_pre,
                                int64_t f_fol, int64_t row_begin,
                                int64_t row_end, int64_t* out_rowids,
                                int64_t* out_i, double* out_d,
                                uint8_t* out_null) {
    int32_t pc[1] = {part_col};
    return bkgpu_window_multi(t, q, pc, part_col >= 0 ? 1 : 0, order,
                              norder, fns, nfns, frame_rows, f_pre, f_fol,
                              row_begin, row_end, out_rowids, out_i, out_d,
                              out_null);
}
