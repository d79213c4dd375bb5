// bkexec.cpp — C++ host execution layer: the ExecNode plugin-surface mirror
// that makes the MI355X engine a drop-in for baikalStore's SELECT pipeline.
//
// The classes here keep the reference's names, signatures, argument meaning
// and error behaviour:
//   ExecNode::init/open/get_next/close      include/exec/exec_node.h:88,140-153
//   ExecNode::create_tree/create_exec_node  src/exec/exec_node.cpp:396-414
//   RuntimeState counters                   include/runtime/runtime_state.h:237-270
//   RowBatch / MemRow containers            include/runtime/row_batch.h:24-231,
//                                           include/mem_row/mem_row.h:28-215
//   ScanNode                                (columnar source; no row mode)
//   FilterNode::get_next (WHERE / HAVING)   src/exec/filter_node.cpp:736-795
//   AggNode::open/get_next                  src/exec/agg_node.cpp:405-587
//   JoinNode (hash equi-join)               src/exec/join_node.cpp, joiner.cpp
//   SortNode::open/get_next (top-N)         src/exec/sort_node.cpp:278-440
//   WindowNode                              src/exec/window_node.cpp
//   LimitNode                               (reached_limit, exec_node.h:186)
//
// Shared pieces: HostCols (the gathered-column block every row-emitting node
// streams from), make_value (one cell -> ExprValue), ExecNode::emit_rows (the
// one get_next loop), ExecNode::n_slots and source_of (what a blocking node
// consumes).
//
// Like the reference's Acero alternative path (region.cpp:2793-2923), the
// blocking nodes compile their subtree into ONE engine pipeline at open()
// and stream materialized rows from get_next() — but the engine here is the
// gfx950 kernel pipeline behind include/bkgpu.h, not a CPU library. There is
// NO row-at-a-time CPU fallback: a plan that reaches ScanNode::get_next in
// row mode returns an error instead of silently computing on the host.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bk_common.h"
#include "../../include/bk_like.h"
#include "../../include/bk_keyenc.h"
#include "../../include/bk_keylayout.h"
#include "../../include/bk_datagen.h"
#include "../../include/bkgpu.h"
#include "../../include/bk_exec.h"

namespace bkexec {

/* ---- ExprValue-lite (include/common/expr_value.h:35-52 tagged union) ---- */
struct ExprValue {
    int32_t type = BK_NULL_TYPE;   /* BkType */
    bool is_null_ = true;
    int64_t i = 0;
    double d = 0.0;
    bool is_null() const { return is_null_; }
};

/* one cell -> ExprValue: a NULL carries no payload, a DOUBLE only d, every
 * other type only i */
static inline ExprValue make_value(int32_t type, bool is_null, int64_t i, double d) {
    ExprValue v;
    v.type = type;
    v.is_null_ = is_null;
    if (!is_null) {
        if (type == BK_DOUBLE) v.d = d;
        else v.i = i;
    }
    return v;
}

/* ---- MemRow (mem_row.h:28-215; one tuple, slot-addressed) ---- */
struct MemRow {
    std::vector<ExprValue> slots;
    explicit MemRow(int n) : slots(n) {}
    const ExprValue& get_value(int slot) const { return slots[slot]; }
    void set_value(int slot, const ExprValue& v) { slots[slot] = v; }
};

/* ---- RowBatch (row_batch.h:24-231) ---- */
class RowBatch {
public:
    explicit RowBatch(size_t capacity = 1024) : _capacity(capacity) {}
    bool is_full() const { return _rows.size() >= _capacity; }
    size_t size() const { return _rows.size(); }
    size_t capacity() const { return _capacity; }
    void set_capacity(size_t c) { _capacity = c; }
    void move_row(std::unique_ptr<MemRow> row) { _rows.emplace_back(std::move(row)); }
    std::unique_ptr<MemRow>& get_row() { return _rows[_idx]; }
    void next() { _idx++; }
    void reset() { _idx = 0; }
    bool is_traverse_over() const { return _idx >= _rows.size(); }
    void clear() { _rows.clear(); _idx = 0; }
    void truncate(size_t n) { if (n < _rows.size()) _rows.resize(n); }
    void drop_range(size_t pos, size_t k) {
        if (k == 0 || pos >= _rows.size()) return;
        size_t end = pos + k < _rows.size() ? pos + k : _rows.size();
        _rows.erase(_rows.begin() + (ptrdiff_t)pos,
                    _rows.begin() + (ptrdiff_t)end);
    }
private:
    std::vector<std::unique_ptr<MemRow>> _rows;
    size_t _idx = 0;
    size_t _capacity;
};

/* ---- RuntimeState (runtime_state.h:83-660 subset: the counters and error
 * surface the store reports back) ---- */
class RuntimeState {
public:
    int64_t num_scan_rows() const { return _num_scan_rows; }
    int64_t num_filter_rows() const { return _num_filter_rows; }
    void inc_num_scan_rows(int64_t n) { _num_scan_rows += n; }
    void inc_num_filter_rows(int64_t n) { _num_filter_rows += n; }
    bool is_cancelled() const { return _cancelled; }
    void cancel() { _cancelled = true; }
    int error_code = 0;
    std::string error_msg;
    size_t row_batch_capacity = 1024;
    int64_t _num_scan_rows = 0;
    int64_t _num_filter_rows = 0;
    bool _cancelled = false;
};

/* ---- ExecNode base (exec_node.h:79-531 subset) ---- */
class ExecNode {
public:
    virtual ~ExecNode() {
        for (auto c : _children) delete c;   /* nodes own children, exec_node.h:83-87 */
    }
    virtual int init(const BkPlanNodeDesc& node) {
        _node_type = node.node_type;
        _limit = node.limit;
        return 0;
    }
    virtual int open(RuntimeState* state) {
        for (auto c : _children) {
            int ret = c->open(state);
            if (ret < 0) return ret;
        }
        return 0;
    }
    virtual int get_next(RuntimeState* state, RowBatch* batch, bool* eos) {
        if (_children.empty()) { *eos = true; return 0; }
        return _children[0]->get_next(state, batch, eos);
    }
    virtual void close(RuntimeState* state) {
        for (auto c : _children) c->close(state);
        _num_rows_returned = 0;
    }
    void add_child(ExecNode* c) { _children.push_back(c); }
    std::vector<ExecNode*>& children() { return _children; }
    bool reached_limit() const {
        return _limit > 0 && _num_rows_returned >= _limit;  /* exec_node.h:186 */
    }
    int32_t node_type() const { return _node_type; }
    /* slots of a row this node emits as the root (0: emits no rows) */
    virtual int n_slots() { return 0; }

    static ExecNode* create_exec_node(const BkPlanNodeDesc& node);
    /* pre-order flattened plan -> tree (exec_node.cpp create_tree) */
    static int create_tree(const BkPlanNodeDesc* nodes, int n, ExecNode** root);

    int32_t _node_type = 0;
    int64_t _limit = -1;
    int64_t _num_rows_returned = 0;
protected:
    /* The get_next loop of every row-emitting node. Per row, in this order:
     * cancelled -> reached_limit -> avail() -> batch full -> fill(row). The
     * source is asked before the batch-full check, so a batch that the last
     * row filled comes back without eos and only the drained call sets it.
     * avail(): 1 = a row is ready (refilling the node's chunk if needed),
     * 0 = drained, < 0 = error (returned as is). fill(row) writes the ready
     * row and advances the node's cursor. */
    template <class Avail, class Fill>
    int emit_rows(RuntimeState* state, RowBatch* batch, bool* eos,
                  Avail&& avail, Fill&& fill) {
        while (true) {
            if (state->is_cancelled()) { *eos = true; return 0; } /* agg_node.cpp:450 */
            if (reached_limit()) { *eos = true; return 0; }
            int r = avail();
            if (r < 0) return r;
            if (r == 0) { *eos = true; return 0; }
            if (batch->is_full()) return 0;
            auto row = std::make_unique<MemRow>(n_slots());
            fill(row.get());
            batch->move_row(std::move(row));
            _num_rows_returned++;
        }
    }
    std::vector<ExecNode*> _children;
private:
    static int build(const BkPlanNodeDesc* nodes, int n, int* pos, ExecNode** out);
};

/* ---- ScanNode: the region's columnar source. Row-mode get_next is an
 * explicit error: the compute path is the GPU pipeline, never host rows. */
class ScanNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _table = node.table;
        if (!_table) return -1;
        return 0;
    }
    int get_next(RuntimeState* state, RowBatch*, bool*) override {
        state->error_msg = "ScanNode row-mode get_next: no CPU fallback; "
                           "plan must be rooted in a GPU-compiled node";
        return -1;
    }
    BkgTable* table() const { return _table; }
private:
    BkgTable* _table = nullptr;
};

template <class V>
static void release(V& v) { V().swap(v); }   /* clear() keeps the capacity */

/* ---- HostCols: the block of gathered columns a row-emitting node streams
 * from — chosen columns of a device table, fetched for a list of row ids
 * (bkgpu_gather) and written into MemRow slots one row at a time. ---- */
class HostCols {
public:
    /* n columns of t: cols[0..n), or columns 0..n-1 when cols is null */
    void bind(BkgTable* t, const int32_t* cols, int n) {
        _table = t;
        _src.resize(n);
        _types.resize(n);
        _i.resize(n);
        _d.resize(n);
        _null.resize(n);
        for (int c = 0; c < n; c++) {
            _src[c] = cols ? cols[c] : c;
            _types[c] = bkgpu_table_col_type(t, _src[c]);
        }
    }
    /* rows rowids[0..n) of every bound column; n == 0 launches nothing */
    int gather(RuntimeState* state, const int64_t* rowids, int64_t n) {
        for (size_t c = 0; c < _src.size(); c++) {
            _i[c].resize(n);
            _d[c].resize(n);
            _null[c].resize(n);
            if (n > 0 &&
                bkgpu_gather(_table, _src[c], rowids, n, _i[c].data(),
                             _d[c].data(), _null[c].data()) != 0) {
                state->error_msg = bkgpu_last_error();
                return -1;
            }
        }
        return 0;
    }
    /* gathered row r -> slots s0 .. s0 + n columns - 1 */
    void write_row(int64_t r, MemRow* row, int s0) const {
        const int n = (int)_types.size();
        for (int c = 0; c < n; c++)
            row->set_value(s0 + c, make_value(_types[c], _null[c][r] != 0,
                                              _i[c][r], _d[c][r]));
    }
    void clear() { *this = HostCols(); }
private:
    BkgTable* _table = nullptr;
    std::vector<int32_t> _src;     /* table column behind each bound column */
    std::vector<int32_t> _types;   /* BkType tags */
    std::vector<std::vector<int64_t>> _i;
    std::vector<std::vector<double>> _d;
    std::vector<std::vector<uint8_t>> _null;
};

/* ---- FilterNode (filter_node.cpp:605-795): holds the conjuncts. When it is
 * an interior node, the blocking parent compiles them into the pipeline;
 * when it is the (effective) root, open() runs the GPU filter and get_next()
 * streams materialized rows. ---- */
class FilterNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _n_conjuncts = node.n_conjuncts;
        memcpy(_conjuncts, node.conjuncts, sizeof(_conjuncts));
        return 0;
    }
    int n_conjuncts() const { return _n_conjuncts; }
    const BkConjunct* conjuncts() const { return _conjuncts; }
    /* the one place a FilterNode's conjuncts become a query's filter */
    void copy_conjuncts(BkQuerySpec* q) const {
        q->n_conjuncts = _n_conjuncts;
        memcpy(q->conjuncts, _conjuncts, sizeof(q->conjuncts));
    }
    bool is_having() const { return _node_type == BK_HAVING_FILTER_NODE; }
    /* As the EFFECTIVE ROOT (SELECT without GROUP BY/ORDER BY) FilterNode
     * emits the passing rows itself (filter_node.cpp:736-795): the GPU
     * filter runs over BOUNDED row-range chunks (BK_FETCH_CHUNK rows,
     * default 4M) and get_next() streams each chunk's survivors before
     * scanning the next range, so host memory stays O(chunk) for a
     * filter-only SELECT over any table size — the streamed analogue of
     * the reference scan's batch iterator (rocksdb_scan_node.cpp
     * get_next loop), not a whole-result materialization.
     * A HAVING_FILTER_NODE root streams the same way over the aggregate's
     * materialized table (source_of): rows in canonical group order, slot
     * layout and type tags of the AGG root. */
    int open(RuntimeState* state) override;
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override;
    int n_slots() override;  /* lazily resolved from the scan's table */
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        _opened = false;
        _eos_source = false;
        _scan_pos = 0;
        _src_table = nullptr;
        release(_rowids);
        _cols.clear();
        _iter = 0;
    }
private:
    int fetch_chunk(RuntimeState* state);  /* 1 = chunk ready, 0 = drained */
    int32_t _n_conjuncts = 0;
    BkConjunct _conjuncts[BK_MAX_CONJUNCTS] = {};
    /* HAVING root: the aggregate's materialized table + every HAVING
     * conjunct of the chain (set by open) */
    BkgTable* _src_table = nullptr;
    BkQuerySpec _src_q{};
    bool _opened = false;
    bool _eos_source = false;
    int _ncols = 0;
    int64_t _nrows = 0;
    int64_t _scan_pos = 0;
    std::vector<int64_t> _rowids;          /* current chunk's survivors */
    HostCols _cols;                        /* ... and their cells */
    int64_t _iter = 0;                     /* cursor within the chunk */
};

/* helpers to locate the pipeline pieces below a blocking node */
static ScanNode* find_scan(ExecNode* n);

/* What a blocking node consumes (SortNode / WindowNode / AggNode / a HAVING
 * root): walking the single-child chain below `node`,
 *  - an AGG_NODE / MERGE_AGG_NODE met before the scan makes the source that
 *    AggNode's materialized table (canonical group order) under the
 *    conjuncts of the HAVING_FILTER_NODEs passed on the way; columns are
 *    then slot indices into [group keys...][agg outputs...];
 *  - a JOIN_NODE makes it the joined table (JoinNode::result_table) under
 *    the WHERE filter passed on the way; columns are then positions in the
 *    join's output list;
 *  - otherwise it is the scan's table under the WHERE filter.
 * Over a materialized source (the first two) the counters stay as the node
 * that produced the table set them — groups and joined rows are not scan
 * rows — and a 0-row table skips the kernels. */
struct Source {
    BkgTable* table = nullptr;
    bool materialized = false;   /* an AggNode's or JoinNode's result table */
    BkQuerySpec q{};          /* only n_conjuncts / conjuncts are set */
};
static int source_of(ExecNode* node, RuntimeState* state, Source* src);

static int64_t fetch_chunk_rows() {
    /* read per chunk (once every few million rows), not cached, so a
     * long-lived process can be re-tuned between queries */
    const char* e = getenv("BK_FETCH_CHUNK");
    int64_t n = e ? atoll(e) : 0;
    return n > 0 ? n : (int64_t)(4 << 20);  /* 4M rows per chunk */
}

int FilterNode::fetch_chunk(RuntimeState* state) {
    BkgTable* t = _src_table;
    if (!t) {
        ScanNode* scan = find_scan(this);
        if (!scan) { state->error_msg = "FilterNode: no scan below"; return -1; }
        t = scan->table();
    }
    if (!_opened) {
        _nrows = bkgpu_table_nrows(t);
        _ncols = bkgpu_table_ncols(t);
        _cols.bind(t, nullptr, _ncols);
        _scan_pos = 0;
        _opened = true;
    }
    BkQuerySpec q{};
    copy_conjuncts(&q);
    if (_src_table) q = _src_q;
    const int64_t chunk = fetch_chunk_rows();
    while (_scan_pos < _nrows) {
        int64_t end = std::min(_nrows, _scan_pos + chunk);
        int64_t span = end - _scan_pos;
        _rowids.resize(span);
        int64_t got = bkgpu_filter_collect(t, &q, _scan_pos, end, span,
                                           _rowids.data());
        if (got < 0) { state->error_msg = bkgpu_last_error(); return -1; }
        _rowids.resize(got);
        /* arrival order: the reference scan emits rows in iterator order;
         * chunks advance in row order, so sorting within the chunk keeps
         * the global stream ordered. */
        std::sort(_rowids.begin(), _rowids.end());
        if (!_src_table) {   /* HAVING-rejected groups are not scan rows */
            state->inc_num_scan_rows(span);
            state->inc_num_filter_rows(span - got);
        }
        _scan_pos = end;
        if (got == 0) continue;
        if (_cols.gather(state, _rowids.data(), got) < 0) return -1;
        _iter = 0;
        return 1;
    }
    _eos_source = true;
    return 0;
}

int FilterNode::get_next(RuntimeState* state, RowBatch* batch, bool* eos) {
    return emit_rows(state, batch, eos,
        [&] {
            if (_iter < (int64_t)_rowids.size()) return 1;
            return _eos_source ? 0 : fetch_chunk(state);
        },
        [&](MemRow* row) { _cols.write_row(_iter++, row, 0); });
}

static ScanNode* find_scan(ExecNode* n) {
    if (!n) return nullptr;
    if (n->node_type() == BK_SCAN_NODE) return static_cast<ScanNode*>(n);
    for (auto c : n->children()) {
        ScanNode* s = find_scan(c);
        if (s) return s;
    }
    return nullptr;
}

struct FetchedGroups {
    int64_t n = 0;
    std::vector<uint8_t> flags;
    std::vector<uint64_t> enc;
    std::vector<int64_t> out_i;
    std::vector<double> out_d;
    std::vector<uint8_t> out_has;
    /* group key k of group g: NULL iff flags bit 7-k; the key word decodes
     * per type (bk_keyenc.h; a STRING key is its dictionary code) */
    ExprValue key(int64_t g, int k, int32_t type) const {
        const uint64_t e = enc[g * BK_MAX_GROUP + k];
        return make_value(type, (flags[g] >> (7 - k)) & 1,
                          type == BK_STRING ? (int64_t)(uint32_t)e : bk_dec_i64(e),
                          bk_dec_f64(e));
    }
    /* aggregate output a of group g (agg-major) */
    ExprValue agg(int64_t g, int a, int32_t type) const {
        const size_t idx = (size_t)a * n + g;
        return make_value(type, !out_has[idx], out_i[idx], out_d[idx]);
    }
};

/* the aggregate results of a run, freed on every exit path */
struct AggOuts {
    std::vector<BkgAggOut*> v;
    AggOuts() = default;
    AggOuts(const AggOuts&) = delete;
    AggOuts& operator=(const AggOuts&) = delete;
    ~AggOuts() { for (auto* o : v) bkgpu_agg_free(o); }
};

/* How an AggNode's outputs come out of engine passes. Without DISTINCT there
 * is one pass, q0 = the node's query. With DISTINCT aggs it is the
 * reference's planner rewrite (agg_node.cpp:247-258): per distinct column j,
 * level 1 (l1[j]) groups by (user keys + that column) and bkgpu_agg_rollup
 * folds the dedup key out under l2[j], which holds only that column's
 * distinct aggs. The reference's MULTI_COUNT_DISTINCT (several distinct
 * columns) runs one such pass per column; every pass shares the same filter
 * and group key, so the canonical-sorted group sets align row for row and
 * the output columns stitch together. Pass 0 (q0) holds the plain aggs and
 * always runs: it anchors the group set when a group has rows but only NULL
 * d values, with a synthetic COUNT(*) if there is no plain agg. */
struct PassPlan {
    struct Src { int pass; int idx; };
    std::vector<Src> src;             /* per aggregate: (pass, index in pass) */
    BkQuerySpec q0{};
    std::vector<BkQuerySpec> l1, l2;  /* per distinct column; pass 1 + j */
    bool has_distinct() const { return !l1.empty(); }
    /* output columns pass p fetches (at least one: the buffers are non-empty) */
    int n_aggs(size_t p) const {
        return std::max(1, p == 0 ? q0.n_aggs : l2[p - 1].n_aggs);
    }
};

/* ---- AggNode (agg_node.cpp:405-587). open() drains the child pipeline —
 * here: compiles {scan, filter, group, aggs} into one bkgpu_filter_agg call
 * (the Acero-slot pattern, region.cpp:2793) — and get_next() emits finalized
 * group rows. MERGE_AGG shares the implementation (the engine's aggregate
 * states already merge, agg_node.cpp:29,539-543). ---- */
class AggNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _desc = node;
        return 0;
    }
    ~AggNode() override { if (_result) bkgpu_table_free(_result); }
    int open(RuntimeState* state) override {
        /* already drained as a table by the node above (result_table) */
        if (_result) return 0;
        return run(state, /*want_table=*/false);
    }
    /* The finished aggregate as a device-resident table of finalized values
     * in canonical group order, slots [group keys...][agg outputs...] —
     * what a HAVING / SORT / WINDOW / AGG node above consumes (source_of).
     * Runs the pipeline open() runs but keeps the result on the device
     * (bkgpu_agg_to_table) instead of fetching it. Lives until close(). */
    BkgTable* result_table(RuntimeState* state) {
        if (!_result && run(state, /*want_table=*/true) < 0) return nullptr;
        return _result;
    }
private:
    /* multi-column DISTINCT stitches its passes on the host: upload the
     * stitched columns as the materialized table */
    int upload_result(RuntimeState* state) {
        const int nc = n_slots();
        const int64_t n = _g.n;
        BkColSpec specs[BK_MAX_GROUP + BK_MAX_AGGS] = {};
        std::vector<std::vector<uint8_t>> valid(nc, std::vector<uint8_t>(n ? n : 1, 1));
        std::vector<std::vector<int64_t>> data(nc, std::vector<int64_t>(n ? n : 1, 0));
        for (int c = 0; c < nc; c++) {
            const int32_t ty = slot_type(c);
            specs[c].col_type = ty;
            int32_t* d32 = (int32_t*)data[c].data();
            for (int64_t g = 0; g < n; g++) {
                const ExprValue v = slot_value(g, c);
                if (v.is_null()) { valid[c][g] = 0; specs[c].null_frac_x1e6 = 1; }
                else if (ty == BK_DOUBLE) memcpy(&data[c][g], &v.d, 8);
                else if (ty == BK_STRING) d32[g] = (int32_t)v.i;
                else data[c][g] = v.i;
            }
        }
        _result = bkgpu_table_create(nc, specs, n);
        if (!_result) { state->error_msg = bkgpu_last_error(); return -1; }
        for (int c = 0; c < nc; c++)
            if (bkgpu_table_upload(_result, c, data[c].data(),
                                   specs[c].null_frac_x1e6 ? valid[c].data()
                                                           : nullptr) != 0) {
                state->error_msg = bkgpu_last_error();
                return -1;
            }
        return 0;
    }
    /* slot s of the output row: [group keys...][agg outputs...] */
    int32_t slot_type(int s) const {
        const int a = s - _q.n_group;
        return a < 0 ? _q.group_types[s]
                     : bk_agg_out_type(_q.aggs[a].agg_type, _q.agg_in_types[a]);
    }
    ExprValue slot_value(int64_t g, int s) const {
        return s < _q.n_group ? _g.key(g, s, slot_type(s))
                              : _g.agg(g, s - _q.n_group, slot_type(s));
    }
    /* _q = the source's filter + this node's group keys and aggregates, with
     * the types resolved against the source table */
    void bind_spec(const Source& source) {
        BkQuerySpec q = source.q;
        q.n_group = _desc.n_group;
        BkgTable* t = source.table;
        for (int k = 0; k < q.n_group; k++) {
            q.group_cols[k] = _desc.group_cols[k];
            q.group_types[k] = bkgpu_table_col_type(t, _desc.group_cols[k]);
            q.group_bits[k] = _desc.group_bits[k];
            q.group_base[k] = _desc.group_base[k];
        }
        q.n_aggs = _desc.n_aggs;
        for (int a = 0; a < q.n_aggs; a++) {
            q.aggs[a] = _desc.aggs[a];
            const BkAggSpec& as = _desc.aggs[a];
            if (as.arith && as.col2 >= 0) {
                /* expression input: DOUBLE domain iff either operand is
                 * DOUBLE (AggFnCall input cast, agg_fn_call.cpp:496-555) */
                int t1 = bkgpu_table_col_type(t, as.col);
                int t2 = bkgpu_table_col_type(t, as.col2);
                q.agg_in_types[a] = (t1 == BK_DOUBLE || t2 == BK_DOUBLE)
                                        ? BK_DOUBLE : BK_INT64;
            } else {
                q.agg_in_types[a] = as.col >= 0
                    ? bkgpu_table_col_type(t, as.col) : BK_INT64;
            }
        }
        _q = q;
    }
    /* which aggregate comes from which pass, and every pass's spec */
    int plan_passes(RuntimeState* state, BkgTable* t, PassPlan* plan) const {
        const BkQuerySpec& q = _q;
        std::vector<int> dcols;            /* distinct columns, deduped */
        std::vector<int> agg_dcol(q.n_aggs, -1);
        for (int a = 0; a < q.n_aggs; a++) {
            if (q.aggs[a].agg_type < BK_AGG_COUNT_DISTINCT) continue;
            int c = q.aggs[a].col;
            size_t j = 0;
            while (j < dcols.size() && dcols[j] != c) j++;
            if (j == dcols.size()) dcols.push_back(c);
            agg_dcol[a] = (int)j;
        }
        plan->src.resize(q.n_aggs);
        plan->q0 = q;
        if (dcols.empty()) {
            for (int a = 0; a < q.n_aggs; a++) plan->src[a] = {0, a};
            return 0;
        }
        if (q.n_group > 2) {
            state->error_msg = "DISTINCT aggs support <= 2 group keys";
            return -1;
        }
        if (q.n_group == 2 && (!q.group_bits[0] || !q.group_bits[1])) {
            /* 2 user keys + d = 3 level-1 keys: they must pack into
             * the two 64-bit key words via declared widths */
            state->error_msg = "DISTINCT with 2 group keys needs "
                               "group_bits declared for both";
            return -1;
        }
        /* aggregate a becomes the next output of pass `pass` under spec p */
        auto place = [&](int a, int pass, BkQuerySpec* p) {
            plan->src[a] = {pass, p->n_aggs};
            p->aggs[p->n_aggs] = q.aggs[a];
            p->agg_in_types[p->n_aggs] = q.agg_in_types[a];
            p->n_aggs++;
        };
        auto count_star_only = [](BkQuerySpec* p) {
            p->aggs[0].agg_type = BK_AGG_COUNT_STAR;
            p->aggs[0].col = -1;
            p->agg_in_types[0] = BK_INT64;
            p->n_aggs = 1;
        };
        BkQuerySpec& q0 = plan->q0;
        q0.n_aggs = 0;
        for (int a = 0; a < q.n_aggs; a++)
            if (agg_dcol[a] < 0) place(a, 0, &q0);
        if (q0.n_aggs == 0) count_star_only(&q0);
        for (size_t j = 0; j < dcols.size(); j++) {
            BkQuerySpec q1 = q;
            q1.n_group = q.n_group + 1;
            q1.group_cols[q.n_group] = dcols[j];
            q1.group_types[q.n_group] = bkgpu_table_col_type(t, dcols[j]);
            if (_desc.distinct_bits > 0) {
                q1.group_bits[q.n_group] = _desc.distinct_bits;
                q1.group_base[q.n_group] = _desc.distinct_base;
            }
            count_star_only(&q1);
            BkQuerySpec q2 = q;
            q2.n_aggs = 0;
            for (int a = 0; a < q.n_aggs; a++)
                if (agg_dcol[a] == (int)j) place(a, (int)j + 1, &q2);
            plan->l1.push_back(q1);
            plan->l2.push_back(q2);
        }
        return 0;
    }
    /* one engine result per pass, in pass order */
    int run_passes(RuntimeState* state, BkgTable* t, int64_t nrows_t,
                   const PassPlan& plan, AggOuts* outs) const {
        const int64_t expected =
            _desc.expected_groups > 0 ? _desc.expected_groups : 65536;
        BkgAggOut* p0 = bkgpu_filter_agg(t, &plan.q0, 0, nrows_t, expected);
        if (!p0) { state->error_msg = bkgpu_last_error(); return -1; }
        outs->v.push_back(p0);
        int32_t src_idx[BK_MAX_AGGS];
        std::fill(src_idx, src_idx + BK_MAX_AGGS, -1);
        for (size_t j = 0; j < plan.l1.size(); j++) {
            /* high-cardinality dedup: try the sort-based level 1 (packs
             * via declared widths or column stats, bkdedup.inc); falls
             * back to the hash path when the shape does not qualify —
             * same results */
            BkgAggOut* l1 = nullptr;
            if (expected * 16 >= (1ll << 22))
                l1 = bkgpu_filter_agg_sorted(t, &plan.l1[j], 0, nrows_t);
            if (!l1)
                l1 = bkgpu_filter_agg(t, &plan.l1[j], 0, nrows_t, expected * 16);
            BkgAggOut* r = l1 ? bkgpu_agg_rollup(l1, &plan.l2[j], src_idx,
                                                 expected) : nullptr;
            if (l1) bkgpu_agg_free(l1);
            if (!r) { state->error_msg = bkgpu_last_error(); return -1; }
            outs->v.push_back(r);
        }
        return 0;
    }
    /* fetch every pass in canonical key order; group sets align (same
     * filter + same user keys), assemble the output columns into _g */
    int fetch_and_stitch(RuntimeState* state, const PassPlan& plan,
                         const AggOuts& outs) {
        const BkQuerySpec& q = _q;
        int64_t n = bkgpu_agg_ngroups(outs.v[0]);
        _g.n = n;
        _g.flags.resize(n ? n : 1);
        _g.enc.resize((n ? n : 1) * BK_MAX_GROUP);
        _g.out_i.resize((size_t)(n ? n : 1) * q.n_aggs);
        _g.out_d.resize((size_t)(n ? n : 1) * q.n_aggs);
        _g.out_has.resize((size_t)(n ? n : 1) * q.n_aggs);
        int64_t got = -1;
        const std::vector<PassPlan::Src>& src = plan.src;
        for (size_t p = 0; p < outs.v.size(); p++) {
            const int pn_aggs = plan.n_aggs(p);
            std::vector<uint8_t> flags(n ? n : 1);
            std::vector<uint64_t> enc((n ? n : 1) * BK_MAX_GROUP);
            std::vector<int64_t> oi((size_t)(n ? n : 1) * pn_aggs);
            std::vector<double> od((size_t)(n ? n : 1) * pn_aggs);
            std::vector<uint8_t> oh((size_t)(n ? n : 1) * pn_aggs);
            int64_t gp = bkgpu_agg_fetch(outs.v[p], /*sorted=*/1, n,
                                         flags.data(), enc.data(), oi.data(),
                                         od.data(), oh.data());
            if (gp < 0 || (p > 0 && gp != got)) {
                state->error_msg = gp < 0 ? bkgpu_last_error()
                                          : "distinct pass group mismatch";
                return -1;
            }
            if (p == 0) {
                got = gp;
                memcpy(_g.flags.data(), flags.data(), (size_t)(gp ? gp : 1));
                memcpy(_g.enc.data(), enc.data(),
                       (size_t)(gp ? gp : 1) * BK_MAX_GROUP * 8);
            }
            for (int a = 0; a < q.n_aggs; a++) {
                if (src[a].pass != (int)p) continue;
                for (int64_t g = 0; g < gp; g++) {
                    size_t di = (size_t)a * gp + g;
                    size_t si = (size_t)src[a].idx * gp + g;
                    _g.out_i[di] = oi[si];
                    _g.out_d[di] = od[si];
                    _g.out_has[di] = oh[si];
                }
            }
        }
        _g.n = got;
        return 0;
    }
    int run(RuntimeState* state, bool want_table) {
        /* resolve the source first: an aggregate below is drained as a
         * table here, so the generic child open() finds it already done */
        Source source;
        if (source_of(this, state, &source) < 0) return -1;
        int ret = ExecNode::open(state);
        if (ret < 0) return ret;
        bind_spec(source);
        BkgTable* t = source.table;
        const int64_t nrows_t = bkgpu_table_nrows(t);
        _g = FetchedGroups{};
        _iter = 0;
        if (source.materialized && nrows_t == 0 && _q.n_group > 0) {
            /* no groups below: empty result, no kernel (without GROUP BY
             * the pipeline still runs: it yields the one all-identity row) */
            return want_table ? upload_result(state) : 0;
        }
        PassPlan plan;
        AggOuts outs;
        if (plan_passes(state, t, &plan) < 0 ||
            run_passes(state, t, nrows_t, plan, &outs) < 0)
            return -1;
        if (!source.materialized) {
            state->inc_num_scan_rows(nrows_t);
            state->inc_num_filter_rows(nrows_t - bkgpu_agg_rows_passed(outs.v[0]));
        }
        if (want_table && !plan.has_distinct()) {
            _result = bkgpu_agg_to_table(outs.v[0], t, /*canonical=*/1);
            if (!_result) state->error_msg = bkgpu_last_error();
            return _result ? 0 : -1;
        }
        if (fetch_and_stitch(state, plan, outs) < 0) return -1;
        return want_table ? upload_result(state) : 0;
    }
public:
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override {
        const int ns = n_slots();
        return emit_rows(state, batch, eos,
            [&] { return _iter < _g.n ? 1 : 0; },
            [&](MemRow* row) {
                for (int s = 0; s < ns; s++)
                    row->set_value(s, slot_value(_iter, s));
                _iter++;
            });
    }
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        _g = FetchedGroups{};
        _iter = 0;
        if (_result) { bkgpu_table_free(_result); _result = nullptr; }
    }
    int n_slots() override { return _desc.n_group + _desc.n_aggs; }
private:
    BkPlanNodeDesc _desc{};
    BkQuerySpec _q{};
    FetchedGroups _g;
    int64_t _iter = 0;
    BkgTable* _result = nullptr;   /* materialized table (result_table) */
};

/* ---- JoinNode (join_node.cpp / joiner.cpp hash join). Two children, each
 * [WHERE ->] SCAN: children[0] is the outer side, children[1] the inner
 * side; a child's WHERE conjuncts restrict that side before the join (the
 * reference pushes such filters below the join's children). run() compiles
 * the subtree into one bkgpu_join call; the result is a device-resident
 * table whose columns are the node's output list, in the order bkgpu_join
 * documents. A node above consumes it through result_table() (source_of);
 * as the root, get_next() streams its rows in result order. ---- */
class JoinNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _desc = node;
        if (node.num_children != 2) return -1;
        if (_desc.n_join_out < 1 || _desc.n_join_out > BK_MAX_COLS) return -1;
        return 0;
    }
    ~JoinNode() override { if (_result) bkgpu_table_free(_result); }
    int open(RuntimeState* state) override {
        if (!_result && run(state) < 0) return -1;
        _nrows = bkgpu_table_nrows(_result);
        _cols.bind(_result, nullptr, n_slots());
        _pos = 0;
        _iter = 0;
        _chunk_n = 0;
        return 0;
    }
    BkgTable* result_table(RuntimeState* state) {
        if (!_result && run(state) < 0) return nullptr;
        return _result;
    }
    int n_slots() override { return _desc.n_join_out; }
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override {
        return emit_rows(state, batch, eos,
            [&] {
                if (_iter < _chunk_n) return 1;
                return _pos < _nrows ? fetch_chunk(state) : 0;
            },
            [&](MemRow* row) { _cols.write_row(_iter++, row, 0); });
    }
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        if (_result) { bkgpu_table_free(_result); _result = nullptr; }
        release(_rowids);
        _cols.clear();
        _nrows = _pos = _iter = _chunk_n = 0;
    }
private:
    /* one side: [WHERE ->] SCAN */
    static int side_of(ExecNode* n, RuntimeState* state, BkgTable** t,
                       BkQuerySpec* q) {
        if (n->node_type() == BK_TABLE_FILTER_NODE ||
            n->node_type() == BK_WHERE_FILTER_NODE) {
            static_cast<FilterNode*>(n)->copy_conjuncts(q);
            n = n->children().empty() ? nullptr : n->children()[0];
        }
        if (!n || n->node_type() != BK_SCAN_NODE) {
            state->error_msg = "JoinNode: each child must be [WHERE ->] SCAN";
            return -1;
        }
        *t = static_cast<ScanNode*>(n)->table();
        return 0;
    }
    int run(RuntimeState* state) {
        if (_children.size() != 2) {
            state->error_msg = "JoinNode needs two children";
            return -1;
        }
        BkgTable *outer = nullptr, *inner = nullptr;
        BkQuerySpec qo{}, qi{};
        if (side_of(_children[0], state, &outer, &qo) < 0 ||
            side_of(_children[1], state, &inner, &qi) < 0)
            return -1;
        BkJoinSpec s{};
        s.join_type = _desc.join_type;
        s.n_keys = _desc.n_join_keys;
        for (int k = 0; k < BK_MAX_JOIN_KEYS; k++) {
            s.outer_key[k] = _desc.join_outer_key[k];
            s.inner_key[k] = _desc.join_inner_key[k];
        }
        s.n_out = _desc.n_join_out;
        for (int c = 0; c < BK_MAX_COLS; c++) {
            s.out_side[c] = _desc.join_out_side[c];
            s.out_col[c] = _desc.join_out_col[c];
        }
        _result = bkgpu_join(outer, &qo, inner, &qi, &s);
        if (!_result) { state->error_msg = bkgpu_last_error(); return -1; }
        /* num_scan_rows: both children's scanned rows */
        const int64_t no = bkgpu_table_nrows(outer);
        state->inc_num_scan_rows(no + bkgpu_table_nrows(inner));
        int64_t st[8];
        if (bkgpu_join_stats(st) == 0) state->inc_num_filter_rows(no - st[0]);
        return 0;
    }
    /* the next fetch_chunk_rows() result rows; 1 = chunk ready */
    int fetch_chunk(RuntimeState* state) {
        const int64_t n = std::min(_nrows - _pos, fetch_chunk_rows());
        _rowids.resize(n);
        for (int64_t i = 0; i < n; i++) _rowids[i] = _pos + i;
        if (_cols.gather(state, _rowids.data(), n) < 0) return -1;
        _pos += n;
        _chunk_n = n;
        _iter = 0;
        return 1;
    }
    BkPlanNodeDesc _desc{};
    BkgTable* _result = nullptr;
    std::vector<int64_t> _rowids;
    HostCols _cols;
    int64_t _nrows = 0, _pos = 0, _iter = 0, _chunk_n = 0;
};

static bool is_agg_node(const ExecNode* n) {
    return n->node_type() == BK_AGG_NODE || n->node_type() == BK_MERGE_AGG_NODE;
}

static int source_of(ExecNode* node, RuntimeState* state, Source* src) {
    FilterNode* where = nullptr;
    int n_having = 0;
    BkConjunct having[BK_MAX_CONJUNCTS];
    for (ExecNode* n = node->children().empty() ? nullptr : node->children()[0];
         n; n = n->children().empty() ? nullptr : n->children()[0]) {
        const int32_t ty = n->node_type();
        if (ty == BK_HAVING_FILTER_NODE) {
            FilterNode* f = static_cast<FilterNode*>(n);
            if (n_having + f->n_conjuncts() > BK_MAX_CONJUNCTS) {
                state->error_msg = "too many HAVING conjuncts";
                return -1;
            }
            for (int i = 0; i < f->n_conjuncts(); i++)
                having[n_having++] = f->conjuncts()[i];
        } else if (ty == BK_TABLE_FILTER_NODE || ty == BK_WHERE_FILTER_NODE) {
            if (!where) where = static_cast<FilterNode*>(n);
        } else if (is_agg_node(n)) {
            src->table = static_cast<AggNode*>(n)->result_table(state);
            if (!src->table) return -1;
            src->materialized = true;
            src->q.n_conjuncts = n_having;
            memcpy(src->q.conjuncts, having, sizeof(BkConjunct) * n_having);
            return 0;
        } else if (ty == BK_JOIN_NODE || ty == BK_SCAN_NODE) {
            if (n_having) {
                state->error_msg = "HAVING_FILTER_NODE without an aggregate below";
                return -1;
            }
            if (ty == BK_JOIN_NODE) {
                /* the joined table; columns above are output-list positions.
                 * A WHERE between the node and the join filters joined rows
                 * (how a non-equi ON condition is applied). */
                src->table = static_cast<JoinNode*>(n)->result_table(state);
                if (!src->table) return -1;
                src->materialized = true;
            } else {
                src->table = static_cast<ScanNode*>(n)->table();
            }
            if (where) where->copy_conjuncts(&src->q);
            return 0;
        }
    }
    state->error_msg = "no scan below";
    return -1;
}

/* the aggregate whose rows a HAVING root re-emits (null if none below) */
static AggNode* agg_below(ExecNode* node) {
    for (ExecNode* n = node; n; n = n->children().empty() ? nullptr : n->children()[0])
        if (is_agg_node(n)) return static_cast<AggNode*>(n);
    return nullptr;
}

int FilterNode::n_slots() {
    if (_ncols == 0) {
        if (is_having()) {
            AggNode* agg = agg_below(this);
            if (agg) _ncols = agg->n_slots();
        } else {
            ScanNode* scan = find_scan(this);
            if (scan) _ncols = bkgpu_table_ncols(scan->table());
        }
    }
    return _ncols;
}

int FilterNode::open(RuntimeState* state) {
    if (is_having()) {
        /* effective-root HAVING: own conjuncts + those of any HAVING below,
         * over the aggregate's materialized table */
        Source source;
        if (source_of(this, state, &source) < 0) return -1;
        if (!source.materialized ||
            source.q.n_conjuncts + _n_conjuncts > BK_MAX_CONJUNCTS) {
            state->error_msg = "HAVING_FILTER_NODE: bad plan below";
            return -1;
        }
        _src_q = source.q;
        for (int i = 0; i < _n_conjuncts; i++)
            _src_q.conjuncts[_src_q.n_conjuncts++] = _conjuncts[i];
        _src_table = source.table;
    }
    return ExecNode::open(state);
}

/* ---- SortNode + TopN (sort_node.cpp:278-440, topn_sorter.h:32-63): open()
 * drains the child via the GPU top-N selection, get_next() emits the
 * materialized out_cols of the selected rows in final order. ---- */
class SortNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _desc = node;
        if (_desc.n_out_cols <= 0) return -1;
        return 0;
    }
    int open(RuntimeState* state) override {
        /* source first (an aggregate below is drained as a table there);
         * above an aggregate, order/out_cols are slot indices, HAVING
         * conjuncts ride in the top-N query and ties fall in canonical
         * group order (the materialized table's arrival order) */
        Source source;
        if (source_of(this, state, &source) < 0) return -1;
        int ret = ExecNode::open(state);
        if (ret < 0) return ret;
        BkQuerySpec q = source.q;
        BkgTable* t = source.table;
        int64_t limit = _limit > 0 ? _limit : bkgpu_table_nrows(t);
        _rowids.resize(limit > 0 ? limit : 1);
        int64_t got = 0;
        if (!(source.materialized && bkgpu_table_nrows(t) == 0))
            got = bkgpu_sort_topk(t, &q, _desc.order, _desc.n_order, 0,
                                  bkgpu_table_nrows(t), limit, _rowids.data());
        if (got < 0) { state->error_msg = bkgpu_last_error(); return -1; }
        _rowids.resize(got);
        if (!source.materialized) state->inc_num_scan_rows(bkgpu_table_nrows(t));
        /* materialize out_cols */
        _cols.bind(t, _desc.out_cols, _desc.n_out_cols);
        if (_cols.gather(state, _rowids.data(), got) < 0) return -1;
        _iter = 0;
        return 0;
    }
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override {
        return emit_rows(state, batch, eos,
            [&] { return _iter < (int64_t)_rowids.size() ? 1 : 0; },
            [&](MemRow* row) { _cols.write_row(_iter++, row, 0); });
    }
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        release(_rowids);
        _cols.clear();
        _iter = 0;
    }
    int n_slots() override { return _desc.n_out_cols; }
private:
    BkPlanNodeDesc _desc{};
    std::vector<int64_t> _rowids;      /* the selected rows, final order */
    HostCols _cols;
    int64_t _iter = 0;
};

/* ---- WindowNode (window_node.cpp, NON-FRAME mode; fns evaluated by
 * bkgpu_window over rows sorted by (partition, order, arrival)). Slots:
 * [out_cols...][window fn outputs...]. ---- */
class WindowNode : public ExecNode {
public:
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _desc = node;
        if (_desc.n_winfns <= 0) return -1;
        return 0;
    }
    static int32_t fn_out_type(const BkWindowFn& f, BkgTable* t) {
        switch (f.fn_type) {
            case BK_WIN_COUNT_STAR: case BK_WIN_COUNT: case BK_WIN_ROW_NUMBER:
            case BK_WIN_RANK: case BK_WIN_DENSE_RANK: case BK_WIN_NTILE:
                return BK_INT64;                 /* window_fn_call.cpp:213-258 */
            case BK_WIN_AVG: case BK_WIN_PERCENT_RANK: case BK_WIN_CUME_DIST:
                return BK_DOUBLE;
            default:
                return bkgpu_table_col_type(t, f.col);  /* input type */
        }
    }
    int open(RuntimeState* state) override {
        /* source first (see SortNode::open); above an aggregate part_col,
         * order, fn inputs and out_cols are slot indices */
        Source source;
        if (source_of(this, state, &source) < 0) return -1;
        int ret = ExecNode::open(state);
        if (ret < 0) return ret;
        BkQuerySpec q = source.q;
        BkgTable* t = source.table;
        int64_t nrows = bkgpu_table_nrows(t);
        _rowids.resize(nrows ? nrows : 1);
        _win_i.resize((size_t)_desc.n_winfns * (nrows ? nrows : 1));
        _win_d.resize((size_t)_desc.n_winfns * (nrows ? nrows : 1));
        _win_n.resize((size_t)_desc.n_winfns * (nrows ? nrows : 1));
        int64_t got = 0;
        if (!(source.materialized && nrows == 0))
            got = bkgpu_window(t, &q, _desc.part_col, _desc.order,
                               _desc.n_order, _desc.winfns, _desc.n_winfns,
                               _desc.frame_mode,
                               _desc.frame_mode ? _desc.frame_pre : -1,
                               _desc.frame_mode ? _desc.frame_fol : -1,
                               0, nrows, _rowids.data(), _win_i.data(),
                               _win_d.data(), _win_n.data());
        if (got < 0) { state->error_msg = bkgpu_last_error(); return -1; }
        _n = got;
        if (!source.materialized) {
            state->inc_num_scan_rows(nrows);
            state->inc_num_filter_rows(nrows - got);
        }
        _fn_types.resize(_desc.n_winfns);
        for (int f = 0; f < _desc.n_winfns; f++)
            _fn_types[f] = fn_out_type(_desc.winfns[f], t);
        /* materialize out_cols of the sorted rows */
        _cols.bind(t, _desc.out_cols, _desc.n_out_cols);
        if (_cols.gather(state, _rowids.data(), _n) < 0) return -1;
        _iter = 0;
        return 0;
    }
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override {
        return emit_rows(state, batch, eos,
            [&] { return _iter < _n ? 1 : 0; },
            [&](MemRow* row) {
                _cols.write_row(_iter, row, 0);
                for (int f = 0; f < _desc.n_winfns; f++) {
                    size_t idx = (size_t)f * _n + _iter;
                    row->set_value(_desc.n_out_cols + f,
                                   make_value(_fn_types[f], _win_n[idx] != 0,
                                              _win_i[idx], _win_d[idx]));
                }
                _iter++;
            });
    }
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        release(_rowids);
        release(_win_i);
        release(_win_d);
        release(_win_n);
        release(_fn_types);
        _cols.clear();
        _iter = 0; _n = 0;
    }
    int n_slots() override { return _desc.n_out_cols + _desc.n_winfns; }

private:
    BkPlanNodeDesc _desc{};
    std::vector<int64_t> _rowids;      /* rows sorted by (partition, order) */
    std::vector<int64_t> _win_i;       /* fn outputs, fn-major */
    std::vector<double> _win_d;
    std::vector<uint8_t> _win_n;
    std::vector<int32_t> _fn_types;
    HostCols _cols;
    int64_t _iter = 0, _n = 0;
};

/* ---- LimitNode (limit_node.cpp): passes the child's rows on, minus the
 * first _offset, up to _limit. ---- */
class LimitNode : public ExecNode {
    int64_t _offset = 0;
    int64_t _num_rows_skipped = 0;
public:
    int n_slots() override {
        return _children.empty() ? 0 : _children[0]->n_slots();
    }
    int init(const BkPlanNodeDesc& node) override {
        ExecNode::init(node);
        _offset = node.offset;
        return 0;
    }
    void close(RuntimeState* state) override {
        ExecNode::close(state);
        _num_rows_skipped = 0;   /* idempotent reset, limit_node.h:16-18 */
    }
    int get_next(RuntimeState* state, RowBatch* batch, bool* eos) override {
        if (_children.empty()) { *eos = true; return 0; }
        if (reached_limit()) { *eos = true; return 0; }
        size_t before = batch->size();
        int ret = _children[0]->get_next(state, batch, eos);
        if (ret < 0) return ret;
        /* OFFSET: drop leading rows until _offset are skipped
         * (limit_node.cpp _num_rows_skipped loop) */
        while (_num_rows_skipped < _offset && batch->size() > before) {
            size_t have = batch->size() - before;
            size_t need = (size_t)(_offset - _num_rows_skipped);
            size_t drop = have < need ? have : need;
            batch->drop_range(before, drop);   /* leading rows of THIS
                                                  child batch only */
            _num_rows_skipped += (int64_t)drop;
            if (batch->size() == before && !*eos) {
                ret = _children[0]->get_next(state, batch, eos);
                if (ret < 0) return ret;
            }
        }
        _num_rows_returned += (int64_t)(batch->size() - before);
        if (_limit > 0 && _num_rows_returned > _limit) {
            /* truncate the overshoot so exactly _limit rows are emitted */
            batch->truncate(batch->size() - (size_t)(_num_rows_returned - _limit));
            _num_rows_returned = _limit;
        }
        if (reached_limit()) *eos = true;
        return 0;
    }
};

/* ---- factory (exec_node.cpp:396-414 switch) ---- */
ExecNode* ExecNode::create_exec_node(const BkPlanNodeDesc& node) {
    switch (node.node_type) {
        case BK_SCAN_NODE:         return new ScanNode();
        case BK_SORT_NODE:         return new SortNode();
        case BK_WINDOW_NODE:       return new WindowNode();
        case BK_AGG_NODE:
        case BK_MERGE_AGG_NODE:    return new AggNode();
        case BK_TABLE_FILTER_NODE:
        case BK_WHERE_FILTER_NODE:
        /* HAVING is a FilterNode too (exec_node.cpp:413); its conjuncts
         * stay above the aggregate (filter_node.cpp:545-550) */
        case BK_HAVING_FILTER_NODE: return new FilterNode();
        case BK_LIMIT_NODE:        return new LimitNode();
        case BK_JOIN_NODE:         return new JoinNode();
        default:                   return nullptr;
    }
}

int ExecNode::build(const BkPlanNodeDesc* nodes, int n, int* pos, ExecNode** out) {
    if (*pos >= n) return -1;
    const BkPlanNodeDesc& d = nodes[*pos];
    (*pos)++;
    ExecNode* node = create_exec_node(d);
    if (!node) return -1;
    if (node->init(d) != 0) { delete node; return -1; }
    for (int c = 0; c < d.num_children; c++) {
        ExecNode* child = nullptr;
        if (build(nodes, n, pos, &child) != 0) { delete node; return -1; }
        node->add_child(child);
    }
    *out = node;
    return 0;
}

int ExecNode::create_tree(const BkPlanNodeDesc* nodes, int n, ExecNode** root) {
    int pos = 0;
    if (build(nodes, n, &pos, root) != 0) return -1;
    if (pos != n) { delete *root; *root = nullptr; return -1; }
    return 0;
}

}  // namespace bkexec

/* ================= C ABI (include/bk_exec.h) ================= */

struct BkExecTree {
    bkexec::ExecNode* root = nullptr;
    bkexec::RuntimeState state;
    bkexec::RowBatch batch;
    bool opened = false;
    bool batch_eos = false;
    int64_t rows_returned = 0;
    ~BkExecTree() { delete root; }
};

static int tree_n_slots(const BkExecTree* t) {
    return t->root ? t->root->n_slots() : 0;
}

extern "C" BkExecTree* bkexec_create_tree(const BkPlanNodeDesc* nodes, int n_nodes) {
    auto* t = new BkExecTree();
    if (bkexec::ExecNode::create_tree(nodes, n_nodes, &t->root) != 0) {
        delete t;
        return nullptr;
    }
    return t;
}

extern "C" int bkexec_open(BkExecTree* t) {
    int ret = t->root->open(&t->state);
    if (ret == 0) t->opened = true;
    return ret;
}

extern "C" int bkexec_n_slots(const BkExecTree* t) { return tree_n_slots(t); }

extern "C" int64_t bkexec_get_next(BkExecTree* t, int64_t capacity,
                                   int32_t* out_tag, int64_t* out_i,
                                   double* out_d, uint8_t* out_null, int* eos) {
    using namespace bkexec;
    if (!t->opened) return -1;
    int n_slots = tree_n_slots(t);
    /* Region::select_normal's driver loop (region.cpp:3166-3216) */
    RowBatch batch((size_t)capacity);
    bool e = false;
    int ret = t->root->get_next(&t->state, &batch, &e);
    if (ret < 0) return ret;
    int64_t out = 0;
    for (batch.reset(); !batch.is_traverse_over(); batch.next(), out++) {
        MemRow* row = batch.get_row().get();
        for (int s = 0; s < n_slots; s++) {
            const ExprValue& v = row->get_value(s);
            int64_t idx = out * n_slots + s;
            out_tag[idx] = v.type;
            out_null[idx] = v.is_null() ? 1 : 0;
            out_i[idx] = v.i;
            out_d[idx] = v.d;
        }
    }
    t->rows_returned += out;
    *eos = e ? 1 : 0;
    return out;
}

extern "C" int64_t bkexec_num_scan_rows(const BkExecTree* t) {
    return t->state.num_scan_rows();
}
extern "C" int64_t bkexec_num_filter_rows(const BkExecTree* t) {
    return t->state.num_filter_rows();
}
extern "C" int64_t bkexec_num_rows_returned(const BkExecTree* t) {
    return t->rows_returned;
}

extern "C" void bkexec_close(BkExecTree* t) {
    if (t->root) t->root->close(&t->state);  /* idempotent reset */
    delete t;
}

extern "C" int bkexec_dict_word(uint64_t dict_seed, int64_t code, char* out,
                                int cap) {
    return bk_dict_word(dict_seed, code, out, cap);
}

/* SQL LIKE export (include/bk_like.h; LikePredicate::like restated) for
 * binding-level pattern->dict-bitmap compilation and the golden tests.
 * Returns 1/0/-1 (-1 = invalid sequence, the reference's boost::none). */
extern "C" int bkgpu_like_match(const char* target, int64_t tlen,
                                const char* pattern, int64_t plen,
                                int charset, char escape_char) {
    return bk_like_match(target, (size_t)tlen, pattern, (size_t)plen,
                         charset, escape_char);
}
extern "C" int bkgpu_like_one(const char* target, int64_t tlen,
                              const char* pattern, int64_t plen,
                              int charset, char escape_char) {
    return bk_like_one(target, (size_t)tlen, pattern, (size_t)plen,
                       charset, escape_char);
}
