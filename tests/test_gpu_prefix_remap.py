# The partition routes' prefix pass and the eager dense scatter's row mapping.
#
# Prefix pass: the histogram kernels add the bucket totals up themselves, one
# scan turns them into bucket bases, and every scatter block reserves its
# range inside a bucket by bumping the bucket's cursor. Record order inside a
# bucket is arrival order, so the same query run twice must still give
# identical integers.
#
# Row mapping: a wave of k_dscatter_e covers 1024 consecutive rows. A wave
# whose whole span is in range deals them out as half-tiles (lane l, pass h ->
# rows 8 * (64 h + l) of the span, pass byte 64 h + l); a wave that crosses
# the range end keeps one 16-row tile per lane and the scalar tail tile. The
# ranges below put the end exactly on, one before and one after a span
# boundary, put both ends off the span grid and inside a half-tile, and leave
# fewer rows than one tile; the block knobs make one block walk many spans
# and many blocks contend for one bucket cursor.
#
# run_route asserts the route by its breakdown names, compares with the CPU
# oracle and requires integer equality with the default dispatch.
import pytest

from tests.test_gpu_routes import (CS, D_DICT, D_SUM16, D_UNI, DENSE, DNS,  # noqa: F401
                                   DPIPE, F64, HASH, I64, K80, PART, PIPE,
                                   S1, S6, STR, Shape, World, _clear_knobs,
                                   assert_same_ints, eng, kid, kn, orc, rid,
                                   run_route, world)

gpu = pytest.mark.gpu

D_ZIPFOCT = 4
N = 300_000      # 292 full wave spans of 1024 rows + 992 rows


def c3(name, p0):
    """The benchmark's mixed shape: two INT64 range predicates and a != on
    the dict key; GROUP BY (octave-Zipf key, 64-code dict); COUNT(*), SUM of
    a narrow int, SUM and AVG of doubles: the NK=2, NAR=1, NF=2 scatter."""
    return Shape(name,
                 [(I64, D_UNI, 0, 1 << 31, 0), (I64, D_UNI, 0, 1 << 31, 0),
                  (I64, D_ZIPFOCT, p0, 0, 0), (I64, D_UNI, 0, 1000, 0),
                  (F64, D_SUM16, 0, 0, 0), (F64, D_SUM16, 0, 0, 0),
                  (STR, D_DICT, 64, 0, 0)],
                 [(0, "<", K80), (1, "<", int((1 << 31) * 0.9)),
                  (6, "!=", 17)],
                 [2, 6], [CS, ("sum", 3), ("sum", 4), ("avg", 5)],
                 n=N, eg=1 << 20, dense=True)


C3_16K = c3("c3_zipfoct16384", 16384)    # 512 range buckets, as the workload
C3_1K = c3("c3_zipfoct1024", 1024)

RANGES = [(0, N), (7, N - 3), (0, 1023), (0, 1024), (0, 1025), (3088, 5144),
          (0, 20)]

DENSE_KNOBS = [dict(), dict(BK_DPART_BLOCKS=1), dict(BK_DPART_BLOCKS=3),
               dict(BK_DPIPE=2), dict(BK_DPIPE=3),
               dict(BK_DABS=1, BK_DABS_MIN=0), dict(BK_DREC_PACK=1),
               dict(BK_NO_DEAGER=1)]


@gpu
@pytest.mark.parametrize("g", DENSE_KNOBS, ids=kid)
@pytest.mark.parametrize("rng", RANGES, ids=rid)
@pytest.mark.parametrize("sh", [C3_16K, C3_1K, S6], ids=repr)
def test_dense_reserve_and_remap(world, monkeypatch, sh, rng, g):
    assert sh.n == N
    run_route(world, monkeypatch, sh, kn(DNS, **g),
              DPIPE if "BK_DPIPE" in g else DENSE, rng=rng)


HASH_KNOBS = [dict(BK_PART_BLOCKS=1), dict(BK_PART_BLOCKS=129),
              dict(BK_PIPE=2), dict(BK_PAIR=1),
              dict(BK_PAIR=1, BK_PART_BLOCKS=1),
              dict(BK_PAIR=1, BK_PART_BLOCKS=129)]


@gpu
@pytest.mark.parametrize("g", HASH_KNOBS, ids=kid)
@pytest.mark.parametrize("rng", [(0, N), (7, N - 3), (0, 1025), (0, 20)],
                         ids=rid)
@pytest.mark.parametrize("sh", [C3_16K, S6, S1], ids=repr)
def test_hash_reserve(world, monkeypatch, sh, rng, g):
    """4096 buckets: most (block, bucket) counts are zero and reserve
    nothing. One block owns every bucket whole; 129 blocks contend."""
    run_route(world, monkeypatch, sh, kn(HASH, BK_PART_P=4096, **g),
              PIPE if "BK_PIPE" in g else PART, rng=rng)


@gpu
@pytest.mark.parametrize("sh", [S1, C3_16K], ids=repr)
def test_hash_reserve_pairs_in_few_buckets(world, monkeypatch, sh):
    """Two buckets, 16 blocks: pairs are the common case, and every block's
    reserved range holds its pairs and its drained leftover."""
    run_route(world, monkeypatch, sh,
              kn(HASH, BK_PAIR=1, BK_PART_P=2, BK_PART_BLOCKS=16), PART,
              rng=(7, N - 3))


TWICE = [(kn(DNS), DENSE), (kn(DNS, BK_DPART_BLOCKS=3), DENSE),
         (kn(DNS, BK_DPIPE=3), DPIPE), (kn(DNS, BK_DREC_PACK=1), DENSE),
         (kn(DNS, BK_NO_DEAGER=1), DENSE),
         (kn(HASH, BK_PART_P=4096, BK_PART_BLOCKS=129), PART),
         (kn(HASH, BK_PART_P=4096, BK_PIPE=2), PIPE),
         (kn(HASH, BK_PAIR=1, BK_PART_P=2, BK_PART_BLOCKS=16), PART)]


@gpu
@pytest.mark.parametrize("knobs,route", TWICE, ids=[kid(k) for k, _ in TWICE])
@pytest.mark.parametrize("sh", [C3_16K, S6], ids=repr)
def test_same_query_twice(world, monkeypatch, sh, knobs, route):
    """Blocks reserve in arrival order, which differs run to run; the
    integer outputs must not."""
    a = run_route(world, monkeypatch, sh, knobs, route, rng=(7, N - 3))
    b = run_route(world, monkeypatch, sh, knobs, route, rng=(7, N - 3))
    assert_same_ints(sh, a, b)
