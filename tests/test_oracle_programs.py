# The CPU oracle's postfix-program evaluator (oracle.c orc_eval_prog) against
# the numpy reference interpreter tests/_exprref.py: every program opcode, as
# an aggregate input and as a conjunct. The GPU route tests take their
# expected values for program aggregates (SUM(if(c > 0, v, 0))) from the
# oracle, so the oracle itself must be pinned by something that is not the
# engine. CPU-only.
import numpy as np
import pytest

from oracle.bindings import make_query
from tests import _exprref as R

TYPE_INT64, TYPE_DOUBLE = 6, 12
A, B, X, V, G = 0, 1, 2, 3, 4
N = 6000
NG = 7


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261020)
    a = rng.integers(-6, 7, N).astype(np.int64)
    a[:8] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1, 7, -7,
             np.iinfo(np.int64).min]
    b = rng.integers(-3, 4, N).astype(np.int64)       # zeros: x/0, x%0
    b[:8] = [-1, -1, 0, 3, 0, -2, 2, 1]
    x = rng.normal(0.0, 2.0, N)
    x[8:12] = [0.0, -0.0, 0.5, -0.5]
    v = rng.integers(0, 1000, N).astype(np.int64)
    g = rng.integers(0, NG, N).astype(np.int64)
    cols = [a, b, x, v, g]
    valids = [(rng.random(N) > 0.15).astype(np.uint8),
              (rng.random(N) > 0.10).astype(np.uint8),
              (rng.random(N) > 0.20).astype(np.uint8), None, None]
    return cols, valids


TYPES = [TYPE_INT64, TYPE_INT64, TYPE_DOUBLE, TYPE_INT64, TYPE_INT64]
_GT0 = ("gt", A, ("liti", 0))
_LT0 = ("lt", A, ("liti", 0))

EXPRS = {
    "div": ("div", A, B),
    "div_double": ("div", X, B),
    "mod": ("mod", A, B),
    "neg_int": ("neg", A),
    "neg_double": ("neg", X),
    "sum_if": ("if", ("gt", B, ("liti", 0)), V, ("liti", 0)),
    "if_mixed": ("if", _GT0, A, X),
    "if_double_cond": ("if", X, B, ("liti", -1)),
    "if_null_branch": ("if", ("isnull", A), ("null",), B),
    "ifnull": ("ifnull", A, B),
    "ifnull_double": ("ifnull", X, ("litf", 0.25)),
    "nullif": ("nullif", B, A),
    "nullif_double": ("nullif", X, ("litf", 0.5)),
    "isnull": ("isnull", X),
    "cmp_eq": ("eq", A, B), "cmp_ne": ("ne", A, B), "cmp_ge": ("ge", A, B),
    "cmp_le_double": ("le", X, B), "cmp_lt": ("lt", A, B),
    "case": ("case", [(_GT0, ("liti", 1)), (_LT0, ("liti", -1))], ("liti", 0)),
    "case_no_else": ("case", [(_GT0, B), (_LT0, X)], None),
    "case_expr": ("case_expr", B, [(("liti", 1), A), (A, X)], None),
    "nested": ("if", ("isnull", A), ("neg", B),
               ("add", ("mod", A, ("ifnull", B, ("liti", 3))), B)),
    "legacy_ops": ("add", ("mul", A, B), ("sub", V, ("liti", 3))),
}


@pytest.mark.parametrize("name", sorted(EXPRS))
def test_program_as_aggregate_input(oracle, data, name):
    """COUNT / SUM / MIN / MAX of the expression per group. COUNT pins the
    nullness, MIN/MAX the exact per-row values, SUM the accumulation (int64
    wraps; DOUBLE within 1e-9 * (sum|x| + 1) of numpy's sum)."""
    cols, valids = data
    expr = EXPRS[name]
    dom, val, x = R.eval_expr(expr, cols, valids)
    # one program per query: BK_MAX_PROG_POOL bounds the ops of a query
    res = {}
    for at in (1, 2, 4, 5):          # COUNT, SUM, MIN, MAX
        q = make_query([], [G], [(0, -1), (at, expr)], TYPES)
        exp = oracle.filter_agg(cols, valids, TYPES, q, nthreads=1)
        assert exp["ngroups"] == NG
        keys = (exp["enc"][:, 0] ^ np.uint64(1 << 63)).astype(np.int64)
        assert np.array_equal(keys, np.arange(NG))
        res[at] = exp
    for g in range(NG):
        m = (cols[G] == g) & val
        assert res[1]["agg_i"][0][g] == int((cols[G] == g).sum())
        assert res[1]["agg_i"][1][g] == int(m.sum())
        has = int(m.any())
        for at in (2, 4, 5):
            assert res[at]["agg_has"][1][g] == has
        if not has:
            continue
        if dom == TYPE_DOUBLE:
            tol = 1e-9 * (np.abs(x[m]).sum() + 1)
            assert abs(res[2]["agg_d"][1][g] - x[m].sum()) <= tol
            assert res[4]["agg_d"][1][g] == x[m].min()
            assert res[5]["agg_d"][1][g] == x[m].max()
        else:
            with np.errstate(over="ignore"):
                s = x[m].astype(np.uint64).sum(dtype=np.uint64)
            assert np.uint64(res[2]["agg_i"][1][g]) == s
            assert res[4]["agg_i"][1][g] == int(x[m].min())
            assert res[5]["agg_i"][1][g] == int(x[m].max())


@pytest.mark.parametrize("name", sorted(EXPRS))
def test_program_as_conjunct(oracle, data, name):
    """WHERE expr > 0 and WHERE expr = 1 (a NULL never passes), in the
    expression's own compare domain."""
    cols, valids = data
    expr = EXPRS[name]
    dom, val, x = R.eval_expr(expr, cols, valids)
    for op, fn in ((2, lambda t: t > 0), (0, lambda t: t == 1)):
        lit = 0 if op == 2 else 1
        q = make_query([(expr, op, dom, float(lit) if dom == TYPE_DOUBLE
                         else lit)], [], [(0, -1)], TYPES)
        exp = oracle.filter_agg(cols, valids, TYPES, q, nthreads=1)
        want = int((val & fn(x)).sum())
        assert exp["rows_passed"] == want
        assert exp["agg_i"][0][0] == want
