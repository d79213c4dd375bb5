# CPU-side checks of the join surface: JoinPlan validation and the right-join
# swap, the C headers (node / join-type values, BkPlanNodeDesc layout: the
# JOIN payload is appended, every earlier field keeps its offset), the ctypes
# mirrors, the exported symbols and the knob's spelling. No compute calls.
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

from tests.test_abi import LIB, REPO, _build_if_needed
from baikaldb_amd.plan import (JoinPlan, BkJoinSpec, LEFT_JOIN, INNER_JOIN,
                               SEMI_JOIN, ANTI_SEMI_JOIN)

I64, F64, STR, DT = 6, 12, 13, 14

# offsetof() of every BkPlanNodeDesc field in the header as it stood before
# the JOIN payload was appended (sizeof was 2296)
OLD_OFFSETS = [
    ("node_type", 0), ("num_children", 4), ("limit", 8), ("offset", 16),
    ("table", 24), ("n_conjuncts", 32), ("conjuncts", 40), ("n_group", 1512),
    ("group_cols", 1516), ("group_bits", 1532), ("group_base", 1552),
    ("n_aggs", 1584), ("aggs", 1588), ("expected_groups", 1784),
    ("distinct_bits", 1792), ("distinct_base", 1800), ("n_order", 1808),
    ("order", 1812), ("n_out_cols", 1876), ("out_cols", 1880),
    ("part_col", 1944), ("n_winfns", 1948), ("winfns", 1952),
    ("frame_mode", 2272), ("frame_pre", 2280), ("frame_fol", 2288),
]
OLD_SIZE = 2296
NEW_FIELDS = ["join_type", "n_join_keys", "join_outer_key", "join_inner_key",
              "n_join_out", "join_out_side", "join_out_col"]


# ---- JoinPlan ---------------------------------------------------------------

def test_join_plan_defaults_and_spec():
    jp = JoinPlan([I64, F64], [I64, STR, I64], [(0, 2)])
    assert jp.join_type == INNER_JOIN and not jp.swapped
    assert jp.out == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    assert jp.out_types == [I64, F64, I64, STR, I64]
    s = jp.to_spec()
    assert (s.join_type, s.n_keys, s.n_out) == (3, 1, 5)
    assert (s.outer_key[0], s.inner_key[0]) == (0, 2)
    assert list(s.out_side)[:5] == [0, 0, 1, 1, 1]
    assert list(s.out_col)[:5] == [0, 1, 0, 1, 2]
    assert JoinPlan([I64], [I64], [(0, 0)], "left").join_type == LEFT_JOIN
    semi = JoinPlan([I64, F64], [I64, I64], [(0, 0)], "semi")
    assert semi.join_type == SEMI_JOIN and semi.out == [(0, 0), (0, 1)]
    anti = JoinPlan([I64], [I64], [(0, 0)], "anti", out=[("outer", 0)])
    assert anti.join_type == ANTI_SEMI_JOIN and anti.out == [(0, 0)]
    two = JoinPlan([DT, I64], [I64, DT], [(0, 1), (1, 0)], "inner", out=[(1, 0)])
    assert two.on == [(0, 1), (1, 0)] and two.to_spec().n_keys == 2


def test_join_plan_right_swaps_sides():
    # a RIGHT JOIN b: kernel outer = b, kernel inner = a, LEFT join; the
    # requested columns (a..., b...) keep their order with sides flipped
    jp = JoinPlan([I64, F64], [STR, I64], [(0, 1)], "right")
    assert jp.swapped and jp.join_type == LEFT_JOIN
    assert jp.on == [(1, 0)]
    assert jp.out == [(1, 0), (1, 1), (0, 0), (0, 1)]
    assert jp.out_types == [I64, F64, STR, I64]
    assert jp.outer_types == [STR, I64] and jp.inner_types == [I64, F64]
    jp = JoinPlan([I64], [I64, I64], [(0, 0)], "right", out=[(1, 1), (0, 0)])
    assert jp.out == [(0, 1), (1, 0)]


@pytest.mark.parametrize("kw", [
    dict(on=[(1, 0)]),                                  # DOUBLE key
    dict(on=[(2, 0)]),                                  # STRING key
    dict(on=[(0, 3)]),                                  # INT64 vs DATETIME
    dict(on=[]),                                        # 0 pairs
    dict(on=[(0, 0)] * 3),                              # 3 pairs
    dict(on=[(0, 9)]),                                  # column out of range
    dict(on=[(0, 0)], out=[(0, 0)] * 17),               # n_out > BK_MAX_COLS
    dict(on=[(0, 0)], out=[]),
    dict(on=[(0, 0)], how="semi", out=[(1, 0)]),        # inner column under SEMI
    dict(on=[(0, 0)], how="anti", out=[(1, 0)]),
    dict(on=[(0, 0)], how="full"),
    dict(on=[(0, 0)], how="cross"),
    dict(on=[(0, 0)], out=[(2, 0)]),                    # bad side
    dict(on=[(0, 0)], out=[(1, 7)]),
])
def test_join_plan_rejects(kw):
    types = [I64, F64, STR, DT]
    with pytest.raises(ValueError):
        JoinPlan(types, types, **kw)


# ---- headers ----------------------------------------------------------------

def _probe_source():
    checks = "\n".join(
        f'typedef char off_{n}[(offsetof(BkPlanNodeDesc, {n}) == {o}) ? 1 : -1];'
        for n, o in OLD_OFFSETS)
    return r'''
#include <stddef.h>
#include "include/bkgpu.h"
#include "include/bk_exec.h"
/* the declarations the header documents, spelled out: a mismatch is a
 * conflicting-types error */
BkgTable* bkgpu_join(BkgTable* outer, const BkQuerySpec* q_outer,
                     BkgTable* inner, const BkQuerySpec* q_inner,
                     const BkJoinSpec* spec);
int bkgpu_join_stats(int64_t out[8]);
typedef char join_node_is_7[(BK_JOIN_NODE == 7) ? 1 : -1];
typedef char jt_null[(BK_NULL_JOIN == 0) ? 1 : -1];
typedef char jt_left[(BK_LEFT_JOIN == 1) ? 1 : -1];
typedef char jt_right[(BK_RIGHT_JOIN == 2) ? 1 : -1];
typedef char jt_inner[(BK_INNER_JOIN == 3) ? 1 : -1];
typedef char jt_semi[(BK_SEMI_JOIN == 4) ? 1 : -1];
typedef char jt_anti[(BK_ANTI_SEMI_JOIN == 5) ? 1 : -1];
typedef char jt_full[(BK_FULL_JOIN == 6) ? 1 : -1];
typedef char scan_is_1[(BK_SCAN_NODE == 1) ? 1 : -1];
typedef char limit_is_11[(BK_LIMIT_NODE == 11) ? 1 : -1];
/* every pre-existing field sits where it sat; the payload is appended */
''' + checks + r'''
typedef char payload_after[(offsetof(BkPlanNodeDesc, join_type) >= ''' + \
        str(OLD_SIZE) + r''') ? 1 : -1];
typedef char spec_size[(sizeof(BkJoinSpec) == ''' + str(C.sizeof(BkJoinSpec)) + r''') ? 1 : -1];
#include <stdio.h>
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BkPlanNodeDesc),
           offsetof(BkPlanNodeDesc, join_type),
           offsetof(BkPlanNodeDesc, n_join_keys),
           offsetof(BkPlanNodeDesc, join_outer_key),
           offsetof(BkPlanNodeDesc, join_inner_key),
           offsetof(BkPlanNodeDesc, n_join_out),
           offsetof(BkPlanNodeDesc, join_out_side),
           offsetof(BkPlanNodeDesc, join_out_col));
    return 0;
}
'''


def test_headers_keep_offsets_and_ctypes_mirror_matches():
    from baikaldb_amd import exec as bx
    assert bx.JOIN == 7
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "probe.c")
        exe = os.path.join(td, "probe")
        with open(src, "w") as f:
            f.write(_probe_source())
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", REPO,
                            src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[:1500]
        out = subprocess.run([exe], capture_output=True, text=True)
        assert out.returncode == 0
    nums = [int(x) for x in out.stdout.split()]
    d = bx.BkPlanNodeDesc
    assert nums[0] == C.sizeof(d)
    assert nums[1:] == [getattr(d, n).offset for n in NEW_FIELDS]
    for name, off in OLD_OFFSETS:
        assert getattr(d, name).offset == off, name


def test_join_node_builder():
    from baikaldb_amd import exec as bx
    d = bx.join_node([I64, F64], [I64, I64], [(0, 1)], "left",
                     out=[(0, 1), (1, 0)])
    assert (d.node_type, d.num_children, d.join_type) == (7, 2, 1)
    assert (d.n_join_keys, d.join_outer_key[0], d.join_inner_key[0]) == (1, 0, 1)
    assert d.n_join_out == 2
    assert [(d.join_out_side[i], d.join_out_col[i]) for i in range(2)] == \
        [(0, 1), (1, 0)]
    with pytest.raises(ValueError):
        bx.join_node([F64], [F64], [(0, 0)])


def test_library_exports_join():
    """Looked up in a child process (see tests/test_postagg_abi.py)."""
    _build_if_needed()
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); "
            "sys.exit(0 if all(hasattr(l, s) for s in sys.argv[2:]) else 1)")
    r = subprocess.run([sys.executable, "-c", code, LIB, "bkgpu_join",
                        "bkgpu_join_stats", "bkgpu_join_stage_ms",
                        "bkgpu_join_tile_rows"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[:400]


def test_python_surface():
    from baikaldb_amd import GpuEngine
    assert callable(GpuEngine.join) and callable(GpuEngine.join_stats)


def test_knob_name_is_read_by_the_engine():
    """The scan of tests/test_gpu_routes.py: a misspelt knob would silently
    test the default route."""
    csrc = os.path.join(REPO, "baikaldb_amd", "csrc")
    text = ""
    for fn in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, fn), errors="replace") as f:
            text += f.read()
    read = set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', text))
    assert "BK_JOIN_LDS_KB" in read
    import tests.test_gpu_join as tj
    assert tj.KNOB == "BK_JOIN_LDS_KB"
