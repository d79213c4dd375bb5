# Post-aggregation on the device: AggResult.to_table (bkgpu_agg_to_table) and
# what runs on the materialized table - HAVING as a conjunct, ORDER BY/LIMIT
# as sort_topk, window functions, re-aggregation, derive_expr.
#
# Section 1 compares to_table with the SAME engine's fetch(sorted=True): the
# finalize kernel and that host code share bk_keylayout.h, so every cell must
# be bit-equal (AVG included - one IEEE division on both sides). Sections 2-4 compare with
# an independent reference: the CPU oracle's filter_agg over the whole row
# range (canonical order) with HAVING / ORDER BY / LIMIT / window /
# re-aggregation applied in numpy, stable sorts so ties fall in canonical
# group order. Materialized tables are built once per shape and only read.
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_agg import DTOL_REL, SEED, eng, orc  # noqa: F401
from tests.test_gpu_merge import (ROUTES, DN, D_KEY, D_NOKEY, _nogroup,  # noqa: F401
                                  _nopass, blob, dec_f64, dec_i64, dworld,
                                  forced, merge, partial, plan_of, scalar,
                                  _blob_cache)
from tests.test_gpu_routes import (I64, F64, STR, S1, S2, S4, SB, S1_20,  # noqa: F401
                                   world, _clear_knobs)

gpu = pytest.mark.gpu


# ---- helpers ----------------------------------------------------------------
def out_type(ct, name, col):
    """bk_agg_out_type (bk_keylayout.h): COUNT* -> INT64, AVG -> DOUBLE, SUM/MIN/MAX
    keep the input domain"""
    if name in ("count_star", "count", "count_distinct"):
        return I64
    if name in ("avg", "avg_distinct"):
        return F64
    if isinstance(col, tuple):
        from baikaldb_amd.plan import compile_expr
        return compile_expr(col, ct, [])
    return ct[col]


def slot_types(ct, group, aggs):
    return [ct[g] for g in group] + [out_type(ct, n, c) for n, c in aggs]


def result_cols(ct, group, aggs, r):
    """a fetch()/oracle result as table columns: [(values, null)] per slot,
    NULL cells 0 (what bkgpu_gather returns for them)"""
    cols = []
    for k, g in enumerate(group):
        null = ((r["flags"] >> (7 - k)) & 1).astype(bool)
        e = r["enc"][:, k].astype(np.uint64)
        if ct[g] == F64:
            v = dec_f64(e)
        elif ct[g] == STR:
            v = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
        else:
            v = dec_i64(e)
        cols.append((np.where(null, np.zeros_like(v), v), null))
    for a, (name, col) in enumerate(aggs):
        null = r["agg_has"][a] == 0
        v = r["agg_d"][a] if out_type(ct, name, col) == F64 else r["agg_i"][a]
        cols.append((np.where(null, np.zeros_like(v), v), null))
    return cols


def gather(e, tab, col, rowids):
    n = len(rowids)
    ids = np.ascontiguousarray(rowids, dtype=np.int64)
    oi, od = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.float64)
    on = np.zeros(max(n, 1), np.uint8)
    rc = e.lib.bkgpu_gather(tab.handle, col,
                            ids.ctypes.data_as(C.POINTER(C.c_int64)), n,
                            oi.ctypes.data_as(C.POINTER(C.c_int64)),
                            od.ctypes.data_as(C.POINTER(C.c_double)),
                            on.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0, e.lib.bkgpu_last_error()
    v = od if tab.col_types[col] == F64 else oi
    return v[:n], on[:n].astype(bool)


def table_cols(e, tab, rowids=None):
    ids = np.arange(tab.nrows, dtype=np.int64) if rowids is None else rowids
    return [gather(e, tab, c, ids) for c in range(len(tab.col_types))]


def bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


def assert_cols_equal(got, want, slots=None):
    assert len(got) == len(want)
    for s in (range(len(want)) if slots is None else slots):
        assert np.array_equal(got[s][1], want[s][1]), f"slot {s} nullness"
        assert np.array_equal(bits(got[s][0]), bits(want[s][0])), f"slot {s}"


def row_matrix(cols, n):
    m = np.zeros((n, 2 * len(cols)), np.uint64)
    for s, (v, null) in enumerate(cols):
        m[:, 2 * s] = bits(v)
        m[:, 2 * s + 1] = null
    return m[np.lexsort(m.T[::-1])] if n else m


def check_to_table(e, res, ct, group, aggs, dict_src=None):
    """to_table == fetch(sorted=True), bit for bit; canonical=False the same
    multiset of rows; validity only where a NULL is; fetch unchanged after"""
    before = res.fetch(sorted=True)
    n = before["ngroups"]
    want = result_cols(ct, group, aggs, before)
    tab = res.to_table(canonical=True, dict_src=dict_src)
    try:
        assert tab.nrows == n == res.ngroups
        assert tab.col_types == slot_types(ct, group, aggs)
        got = table_cols(e, tab)
        assert_cols_equal(got, want)
        assert tab.col_nullable == [bool(null.any()) for _, null in want]
        for a, (name, _) in enumerate(aggs):
            if name.startswith("count"):
                assert not tab.col_nullable[len(group) + a]
    finally:
        tab.free()
    raw = res.to_table(canonical=False)
    try:
        assert raw.nrows == n and raw.col_types == slot_types(ct, group, aggs)
        assert np.array_equal(row_matrix(table_cols(e, raw), n),
                              row_matrix(want, n))
    finally:
        raw.free()
    after = res.fetch(sorted=True)
    for k in ("flags", "enc", "agg_i", "agg_d", "agg_has"):
        assert np.array_equal(before[k], after[k]), k
    assert after["rows_passed"] == before["rows_passed"]
    return before


# ---- 1. to_table == fetch(sorted=True) --------------------------------------
T1 = [(sh, r) for sh in (S1, S2, S4, SB[True])
      for r in ("FUSED", "PART", "DENSE", "SORTED")
      if r != "DENSE" or sh.dense]


@gpu
@pytest.mark.parametrize("sh,route", T1, ids=[f"{s}-{r}" for s, r in T1])
def test_to_table_equals_fetch(world, monkeypatch, sh, route):
    # the fused route is forced by expected_groups <= 512: half the rows, as
    # the merge matrix runs it (fewer 4x regrows)
    re_ = sh.n // 2 + 1 if route == "FUSED" else sh.n
    res = partial(world, monkeypatch, sh, route, 0, re_)
    try:
        got = check_to_table(world.eng, res, sh.ct, sh.group, sh.aggs,
                             dict_src=world.table(sh))
    finally:
        res.free()
    assert got["ngroups"] > 1000


@gpu
def test_to_table_of_merged_empty_destination(world, monkeypatch):
    sh = S2
    m = sh.n // 2 + 1
    a = partial(world, monkeypatch, sh, "EMPTY", 0, 0)
    try:
        merge(a, blob(world, monkeypatch, sh, "PART", 0, m))
        merge(a, blob(world, monkeypatch, sh, "SORTED", m, sh.n))
        got = check_to_table(world.eng, a, sh.ct, sh.group, sh.aggs)
    finally:
        a.free()
    exp = world.expected(monkeypatch, sh, 0, sh.n)
    assert got["ngroups"] == exp["ngroups"]
    assert np.array_equal(got["agg_i"][0], exp["agg_i"][0])


@gpu
@pytest.mark.parametrize("sh", [D_KEY, D_NOKEY], ids=repr)
def test_to_table_of_rollup_output(dworld, monkeypatch, sh):
    """COUNT/SUM(DISTINCT) states are COUNT-/SUM-shaped"""
    l1 = dworld.level1(monkeypatch, sh, "PART", 0, DN)
    r = None
    try:
        r = dworld.rollup(sh, l1)
        got = check_to_table(dworld.eng, r, sh.ct, sh.group, sh.aggs)
    finally:
        l1.free()
        if r is not None:
            r.free()
    exp = dworld.expected(sh)
    assert got["ngroups"] == (exp["ngroups"] if sh.group else 1)
    assert np.array_equal(got["agg_i"][1], exp["agg_i"][1])


@gpu
@pytest.mark.parametrize("nopass", [False, True])
def test_to_table_without_group_by(world, monkeypatch, nopass):
    """n_group == 0: one row, no key columns; with no passing row SUM / AVG /
    MIN / MAX are NULL cells and COUNT is 0"""
    sh = _nogroup(S2, 300_000)
    res = scalar(world, monkeypatch, sh, 0, sh.n, nopass=nopass)
    try:
        got = check_to_table(world.eng, res, sh.ct, sh.group, sh.aggs)
    finally:
        res.free()
    assert got["ngroups"] == 1
    assert list(got["agg_has"][:, 0]) == ([1, 1, 0, 0, 0, 0] if nopass
                                          else [1] * 6)


@gpu
def test_to_table_zero_groups(world, monkeypatch):
    """a grouped query whose filter passes no row: a valid 0-row table that
    the consumers accept"""
    from baikaldb_amd import QueryPlan
    sh = S1
    t, plan = plan_of(world, _nopass(sh))
    e = world.eng
    res = forced(monkeypatch, {}, lambda: e.filter_agg(t, plan,
                                                       expected_groups=sh.eg))
    try:
        assert res.ngroups == 0
        check_to_table(e, res, sh.ct, sh.group, sh.aggs)
        tab = res.to_table()
        try:
            assert tab.nrows == 0 and tab.col_nullable == [False] * 5
            assert len(e.sort_topk(tab, [(1, 0, 0)], 10)) == 0
            again = e.filter_agg(tab, QueryPlan(tab.col_types, group=[1],
                                                aggs=[("count_star", -1)]))
            try:
                assert again.ngroups == 0
            finally:
                again.free()
        finally:
            tab.free()
    finally:
        res.free()


@gpu
def test_to_table_20_rows(world, monkeypatch):
    sh = S1_20
    t, plan = plan_of(world, sh)
    res = forced(monkeypatch, {}, lambda: world.eng.filter_agg(
        t, plan, expected_groups=sh.eg))
    try:
        got = check_to_table(world.eng, res, sh.ct, sh.group, sh.aggs)
    finally:
        res.free()
    exp = world.expected(monkeypatch, sh, 0, sh.n)
    assert 0 < got["ngroups"] == exp["ngroups"] <= 20


@gpu
def test_to_table_copies_dictionary(eng):
    """BK_STRING key and MIN/MAX columns carry dict_src's dictionary"""
    from baikaldb_amd import QueryPlan
    words = ["pear", "apple", "fig", "apple", "kiwi", "fig", "pear", "apple"]
    t = eng.create_table([(STR, 2, 8, 0, 0), (I64, 0, 0, 10, 0)], len(words))
    try:
        eng.upload_strings(t, 0, words)
        eng.upload(t, 1, np.arange(len(words), dtype=np.int64))
        plan = QueryPlan(t.col_types, group=[0],
                         aggs=[("count_star", -1), ("max", 0), ("sum", 1)])
        res = eng.filter_agg(t, plan, expected_groups=16)
        try:
            tab = res.to_table(dict_src=t)
            bare = res.to_table()
        finally:
            res.free()
        try:
            assert tab.col_types == [STR, I64, STR, I64]
            cols = table_cols(eng, tab)
            uniq = sorted(set(words))
            for c in (0, 2):
                assert [eng.dict_word(tab, c, int(k)) for k in cols[c][0]] \
                    == uniq
            assert list(cols[1][0]) == [words.count(w) for w in uniq]
            assert eng.dict_word(bare, 0, 0) is None
        finally:
            tab.free()
            bare.free()
    finally:
        t.free()


# ---- numpy reference for sections 2-4 ---------------------------------------
_CMP = {"=": np.equal, "!=": np.not_equal, ">": np.greater,
        ">=": np.greater_equal, "<": np.less, "<=": np.less_equal}


def np_having(cols, conj):
    """ternary logic: a NULL operand is not true; or_group members OR
    together, clauses AND together"""
    n = len(cols[0][0])
    keep = np.ones(n, bool)
    groups = {}
    for cj in conj:
        v, null = cols[cj[0]]
        m = ~null & _CMP[cj[1]](v, cj[2])
        og = cj[3] if len(cj) > 3 else 0
        if og:
            groups[og] = groups.get(og, np.zeros(n, bool)) | m
        else:
            keep &= m
    for m in groups.values():
        keep &= m
    return keep


def np_order(cols, keep, order, limit=None):
    """row ids of the kept rows under ORDER BY (slot, asc, null_first), NULLs
    first or last regardless of direction, ties in row (canonical) order"""
    idx = np.nonzero(keep)[0]
    keys = []
    for slot, asc, nf in order:
        v, null = cols[slot][0][idx], cols[slot][1][idx]
        r = np.unique(v, return_inverse=True)[1].astype(np.int64).reshape(-1)
        r = np.where(null, 0, r if asc else -r)
        keys += [np.where(null, 0 if nf else 2, 1), r]
    out = idx[np.lexsort(tuple(reversed(keys)))] if keys else idx
    return out if limit is None else out[:limit]


class Mat:
    """materialized default-route result + oracle columns, once per shape"""

    def __init__(self):
        self.d = {}

    def get(self, world, monkeypatch, sh):
        if sh.name not in self.d:
            exp = world.expected(monkeypatch, sh, 0, sh.n)
            t, plan = plan_of(world, sh)
            res = forced(monkeypatch, {}, lambda: world.eng.filter_agg(
                t, plan, expected_groups=sh.eg))
            try:
                tab = res.to_table(dict_src=t)
            finally:
                res.free()
            ocols = result_cols(sh.ct, sh.group, sh.aggs, exp)
            for v, null in ocols:
                v.setflags(write=False)
                null.setflags(write=False)
            assert tab.nrows == exp["ngroups"]
            self.d[sh.name] = (tab, ocols)
        return self.d[sh.name]

    def close(self):
        for tab, _ in self.d.values():
            tab.free()
        self.d.clear()


@pytest.fixture(scope="module")
def mat(world):
    m = Mat()
    yield m
    m.close()


def run_query(e, tab, conj, order, limit):
    from baikaldb_amd import QueryPlan
    return e.sort_topk(tab, order, limit,
                       plan=QueryPlan(tab.col_types, conjuncts=conj))


# slots compared bit for bit against the oracle: everything but DOUBLE
# SUM/AVG (reduction order differs; section 3)
def exact_slots(sh):
    ng = len(sh.group)
    return [s for s in range(ng + len(sh.aggs))
            if s < ng or not (sh.aggs[s - ng][0] in ("sum", "avg") and
                              out_type(sh.ct, *sh.aggs[s - ng]) == F64)]


# S1 slots: 0 key | 1 count | 2 sum | 3 min | 4 max
# S2 slots: 0 key | 1 dict key | 2 count(*) | 3 count | 4 sum (nullable)
#           | 5 avg f64 | 6 min | 7 max f64
# S4 slots: 0 key (nullable) | 1 count | 2 sum | 3 min | 4 count
Q2 = {
    "having_order_limit10": (S1, [(1, ">=", 3)], [(2, 0, 0), (0, 1, 1)], 10),
    "limit_above_survivors": (S1, [(1, ">=", 40)], [(2, 0, 0), (0, 1, 1)],
                              100_000),
    "or_group_pair": (S1, [(1, ">=", 5, 1), (4, ">=", 990, 1),
                           (0, "<", 50_000)], [(3, 1, 1), (0, 0, 0)], 500),
    "tie_break_count_desc": (S1, [], [(1, 0, 0)], 1000),
    "null_key_first": (S4, [], [(0, 1, 1)], 50),
    "null_key_last_desc": (S4, [(1, ">=", 2)], [(0, 0, 0)], 100_000),
    "null_key_rejected_by_having": (S4, [(0, ">=", 0)], [(1, 0, 0), (0, 1, 1)],
                                    100_000),
    "null_sum_first": (S2, [], [(4, 0, 1), (0, 1, 1), (1, 1, 1)], 300),
    "null_sum_last": (S2, [(2, ">=", 2)], [(4, 1, 0), (0, 0, 1), (1, 1, 1)],
                      100_000),
    "null_sum_rejected_by_having": (S2, [(4, ">=", 0)],
                                    [(6, 1, 1), (0, 1, 1), (1, 1, 1)], 300),
}


@gpu
@pytest.mark.parametrize("case", sorted(Q2))
def test_having_order_limit_exact(world, monkeypatch, mat, case):
    sh, conj, order, limit = Q2[case]
    tab, ocols = mat.get(world, monkeypatch, sh)
    keep = np_having(ocols, conj)
    want = np_order(ocols, keep, order, limit)
    # the cases must exercise what they are named for
    if case == "limit_above_survivors":
        assert 0 < keep.sum() < limit
    if case == "tie_break_count_desc":
        v = ocols[1][0][want]
        assert len(want) == 1000 and (np.diff(v) == 0).sum() > 500
        # the cut itself falls inside a run of equal counts
        assert (ocols[1][0] == v[-1]).sum() > (v == v[-1]).sum()
    if case.startswith("null_key"):
        assert ocols[0][1].sum() == 1
        nullrow = int(np.nonzero(ocols[0][1])[0][0])
        if case == "null_key_first":
            assert want[0] == nullrow
        elif case == "null_key_last_desc":
            assert want[-1] == nullrow and len(want) < limit
        else:
            assert nullrow not in want and len(want) == tab.nrows - 1
    if case.startswith("null_sum"):
        nn = int(ocols[4][1].sum())
        assert nn > 1000
        if case == "null_sum_first":
            assert ocols[4][1][want].all()
        elif case == "null_sum_last":
            assert ocols[4][1][want[-1]] and not ocols[4][1][want[0]]
        else:
            assert keep.sum() == tab.nrows - nn
    got = run_query(world.eng, tab, conj, order, limit)
    assert np.array_equal(got, want)
    slots = exact_slots(sh)
    assert_cols_equal(table_cols(world.eng, tab, got),
                      [(v[want], null[want]) for v, null in ocols], slots)


# ---- 3. HAVING / ORDER BY on an inexact DOUBLE aggregate ---------------------
def avg_bound(sh, ocols, slot, count_slot):
    """assert_parity's bound for a DOUBLE SUM/AVG cell"""
    return DTOL_REL * (np.abs(ocols[slot][0]) +
                       np.maximum(ocols[count_slot][0], 1))


@gpu
def test_having_on_double_avg_at_widest_gap(world, monkeypatch, mat):
    """The two sides may differ by DTOL_REL * (|avg| + count). The literal is
    the midpoint of the widest gap between adjacent oracle values, so no
    value within its bound of the oracle's can fall on the other side.
    (S2: gap 3.8e-2 against bounds of 4e-10, checked with the oracle alone.)"""
    sh = S2
    tab, ocols = mat.get(world, monkeypatch, sh)
    avg, null = ocols[5]
    assert not null.any()
    b = avg_bound(sh, ocols, 5, 2)
    o = np.argsort(avg, kind="stable")
    gaps = np.diff(avg[o])
    j = int(np.argmax(gaps))
    assert gaps[j] / 2 > 100 * max(b[o[j]], b[o[j + 1]])       # precondition
    lit = float((avg[o[j]] + avg[o[j + 1]]) / 2)
    for op in (">", "<="):
        keep = np_having(ocols, [(5, op, lit)])
        assert 0 < keep.sum() < len(avg)
        got = run_query(world.eng, tab, [(5, op, lit)],
                        [(0, 1, 1), (1, 1, 1)], tab.nrows)
        # non-NULL keys: (key, dict key) ascending IS canonical order
        assert np.array_equal(got, np.nonzero(keep)[0]), op


@gpu
def test_order_by_double_avg_desc_limit50(world, monkeypatch, mat):
    """ORDER BY avg DESC LIMIT 50: the first L rows by key, L the longest
    prefix whose adjacent oracle gaps all exceed 100x the bound (S2: L = 43,
    checked with the oracle alone)"""
    sh = S2
    tab, ocols = mat.get(world, monkeypatch, sh)
    avg = ocols[5][0]
    b = avg_bound(sh, ocols, 5, 2)
    want = np_order(ocols, np.ones(len(avg), bool), [(5, 0, 0)], 51)
    gap = -np.diff(avg[want])
    ok = gap > 100 * np.maximum(b[want][:-1], b[want][1:])
    L = 50 if ok.all() else int(np.argmin(ok))
    assert L >= 10                                             # precondition
    got = run_query(world.eng, tab, [], [(5, 0, 0)], 50)
    assert len(got) == 50
    assert np.array_equal(got[:L], want[:L])
    gk = table_cols(world.eng, tab, got[:L])
    assert_cols_equal(gk, [(v[want[:L]], n_[want[:L]]) for v, n_ in ocols],
                      [0, 1])
    err = np.abs(gk[5][0] - avg[want[:L]])
    assert np.all(err <= b[want[:L]])


# ---- 4. composition ----------------------------------------------------------
@gpu
def test_window_over_materialized_result(world, monkeypatch, mat):
    """rank / row_number / sum() over (partition by count order by sum desc)
    on S1's groups"""
    sh = S1
    tab, ocols = mat.get(world, monkeypatch, sh)
    part, key = ocols[1][0], ocols[2][0]
    n = len(part)
    got = world.eng.window(tab, [("rank", -1), ("row_number", -1), ("sum", 2)],
                           part_col=1, order=[(2, 0, 0)])
    perm = np.lexsort((np.arange(n), -key, part))
    ps, ks = part[perm], key[perm]
    pos = np.arange(n)
    new_part = np.r_[True, ps[1:] != ps[:-1]]
    new_run = new_part | np.r_[True, ks[1:] != ks[:-1]]
    pstart = np.maximum.accumulate(np.where(new_part, pos, 0))
    rstart = np.maximum.accumulate(np.where(new_run, pos, 0))
    totals = np.add.reduceat(ks, np.nonzero(new_part)[0])
    assert got["n"] == n and new_part.sum() > 20
    assert np.array_equal(got["rowids"], perm)
    assert not got["out_null"].any()
    assert np.array_equal(got["out_i"][0], rstart - pstart + 1)
    assert np.array_equal(got["out_i"][1], pos - pstart + 1)
    assert np.array_equal(got["out_i"][2], totals[np.cumsum(new_part) - 1])


@gpu
@pytest.mark.parametrize("how", ["filter_agg", "filter_agg_sorted"])
def test_reaggregate_group_by_count(world, monkeypatch, mat, how):
    """SELECT c, COUNT(*), SUM(s), MAX(k) FROM (S1's result) WHERE c >= 2
    GROUP BY c - the materialized table has no validity arrays, so it is an
    ordinary NULL-free input to either aggregate entry point"""
    from baikaldb_amd import QueryPlan
    sh = S1
    tab, ocols = mat.get(world, monkeypatch, sh)
    assert tab.col_nullable == [False] * 5
    plan = QueryPlan(tab.col_types, conjuncts=[(1, ">=", 2)], group=[1],
                     aggs=[("count_star", -1), ("sum", 2), ("max", 0)])
    e = world.eng
    res = forced(monkeypatch, {}, lambda: (
        e.filter_agg(tab, plan, expected_groups=1 << 10) if how == "filter_agg"
        else e.filter_agg_sorted(tab, plan)))
    try:
        got = res.fetch(sorted=True)
    finally:
        res.free()
    keep = ocols[1][0] >= 2
    c, s, k = ocols[1][0][keep], ocols[2][0][keep], ocols[0][0][keep]
    uc, inv = np.unique(c, return_inverse=True)
    inv = inv.reshape(-1)
    mx = np.full(len(uc), np.iinfo(np.int64).min)
    np.maximum.at(mx, inv, k)
    assert got["rows_passed"] == keep.sum() and got["ngroups"] == len(uc) > 20
    assert not got["flags"].any() and got["agg_has"].all()
    assert np.array_equal(dec_i64(got["enc"][:, 0].astype(np.uint64)), uc)
    assert np.array_equal(got["agg_i"][0], np.bincount(inv))
    assert np.array_equal(got["agg_i"][1],
                          np.bincount(inv, weights=s).astype(np.int64))
    assert np.array_equal(got["agg_i"][2], mx)


@gpu
def test_order_by_expression_of_aggregates(world, monkeypatch):
    """ORDER BY SUM(v) / COUNT(*) DESC, k LIMIT 20 HAVING that ratio > 600:
    derive_expr on the materialized table. Both operands are exact integers
    below 2^53 and the divide is one IEEE f64 operation on either side, so
    the comparison is exact."""
    sh = S1
    exp = world.expected(monkeypatch, sh, 0, sh.n)
    ocols = result_cols(sh.ct, sh.group, sh.aggs, exp)
    t, plan = plan_of(world, sh)
    e = world.eng
    res = forced(monkeypatch, {}, lambda: e.filter_agg(t, plan,
                                                       expected_groups=sh.eg))
    try:
        tab = res.to_table()
    finally:
        res.free()
    try:
        nc = e.derive_expr(tab, ("div", 2, 1))
        assert nc == 5 and tab.col_types[5] == F64
        ratio = ocols[2][0].astype(np.float64) / ocols[1][0].astype(np.float64)
        cols = ocols + [(ratio, np.zeros(len(ratio), bool))]
        conj, order = [(5, ">", 600.0)], [(5, 0, 0), (0, 1, 1)]
        keep = np_having(cols, conj)
        assert 20 < keep.sum() < len(ratio)
        want = np_order(cols, keep, order, 20)
        got = run_query(e, tab, conj, order, 20)
        assert np.array_equal(got, want)
        assert_cols_equal(table_cols(e, tab, got),
                          [(v[want], n_[want]) for v, n_ in cols])
    finally:
        tab.free()
