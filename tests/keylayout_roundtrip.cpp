// Stand-alone host check of include/bk_keylayout.h: layouts against values
// worked out by hand, get(put(e)) == e at the edges of every field (the
// shifts at width 64 are the point), and bk_agg_finalize on one hand-written
// state per aggregate kind and input type. Built and run by
// tests/test_keylayout_host.py; exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "bk_common.h"
#include "bk_keylayout.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            g_fail++;                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
        }                                                       \
    } while (0)

struct Case {
    const char* name;
    int n;
    int32_t bits[BK_MAX_GROUP];     /* declared: 0 = full word */
    int32_t type[BK_MAX_GROUP];
    int64_t base[BK_MAX_GROUP];
    /* by hand */
    int nwords;
    int32_t shift[BK_MAX_GROUP];
    int32_t word[BK_MAX_GROUP];
};

#define I BK_INT64
#define S BK_STRING
static const Case CASES[] = {
    {"[] 1 key",     1, {0},            {I},          {-9},
     1, {0},          {0}},
    {"[] 2 keys",    2, {0, 0},         {I, S},       {-9, 5},
     2, {0, 0},       {0, 1}},
    {"[10,6,10]",    3, {10, 6, 10},    {I, S, I},    {-3, 2, -500},
     1, {0, 10, 16},  {0, 0, 0}},
    {"[10,6,10,0]",  4, {10, 6, 10, 0}, {I, S, I, I}, {-3, 2, -500, -77},
     2, {0, 10, 16, 0}, {0, 0, 0, 1}},
    {"[33,31,0]",    3, {33, 31, 0},    {I, I, S},    {-1, -500, 4},
     2, {0, 33, 0},   {0, 0, 1}},
    {"[40,30,8]",    3, {40, 30, 8},    {I, I, S},    {-1, -500, 4},
     2, {0, 0, 30},   {0, 1, 1}},
    {"[0,20]",       2, {0, 20},        {I, I},       {-8, -100000},
     2, {0, 0},       {0, 1}},
    {"[63]",         1, {63},           {I},          {-500},
     1, {0},          {0}},
    {"[1,63,1,63]",  4, {1, 63, 1, 63}, {I, I, S, I}, {-1, -500, 7, -12},
     2, {0, 1, 0, 1}, {0, 0, 1, 1}},
};
/* more words than the engine holds: only the walk is checked. (Five keys
 * exceed BK_MAX_GROUP == 4; four keys reach three words.) */
static const Case THREE_WORDS =
    {"[33,31,40,40]", 4, {33, 31, 40, 40}, {I, I, I, I}, {-4, -1, -2, -3},
     3, {0, 33, 0, 0}, {0, 0, 1, 2}};
#undef I
#undef S

static BkQuerySpec spec_of(const Case& c) {
    static BkQuerySpec q;   /* large: keep it off the stack */
    memset(&q, 0, sizeof q);
    q.n_group = c.n;
    for (int k = 0; k < c.n; k++) {
        q.group_cols[k] = k;
        q.group_types[k] = c.type[k];
        q.group_bits[k] = c.bits[k];
        q.group_base[k] = c.base[k];
    }
    return q;
}

static void check_walk(const Case& c, const BkKeyLayout& l) {
    CHECK(l.n == c.n, "%s: n %d", c.name, l.n);
    CHECK(l.nwords == c.nwords, "%s: nwords %d want %d", c.name, l.nwords,
          c.nwords);
    for (int k = 0; k < c.n; k++) {
        CHECK(l.bits[k] == (c.bits[k] ? c.bits[k] : 64), "%s: bits[%d] %d",
              c.name, k, l.bits[k]);
        CHECK(l.shift[k] == c.shift[k], "%s: shift[%d] %d want %d", c.name, k,
              l.shift[k], c.shift[k]);
        CHECK(l.word[k] == c.word[k], "%s: word[%d] %d want %d", c.name, k,
              l.word[k], c.word[k]);
    }
}

/* smallest / largest encoding key k can hold, independent of the header's
 * own mask helper */
static uint64_t enc_lo(const Case& c, int k) {
    if (c.bits[k] == 0) return 0;
    return c.type[k] == BK_STRING ? (uint64_t)c.base[k]
                                  : ((uint64_t)c.base[k] ^ (1ull << 63));
}
static uint64_t enc_span(const Case& c, int k) {   /* hi - lo */
    if (c.bits[k] == 0) return ~0ull;
    return (1ull << c.bits[k]) - 1;     /* declared bits are 1..63 */
}

static void check_round_trip(const Case& c, const BkKeyLayout& l,
                             std::mt19937_64& rng) {
    /* rounds 0/1: every key at its minimum / maximum; then 1000 random */
    for (int round = 0; round < 1002; round++) {
        uint64_t e[BK_MAX_GROUP], k0 = 0, k1 = 0;
        for (int k = 0; k < c.n; k++) {
            const uint64_t off = round == 0 ? 0
                               : round == 1 ? enc_span(c, k)
                                            : (rng() & enc_span(c, k));
            e[k] = enc_lo(c, k) + off;
            bk_key_put(&l, k, e[k], &k0, &k1);
        }
        for (int k = 0; k < c.n; k++) {
            const uint64_t g = bk_key_get(&l, k, k0, k1, 0);
            CHECK(g == e[k], "%s: round %d key %d got %llx want %llx", c.name,
                  round, k, (unsigned long long)g, (unsigned long long)e[k]);
        }
        /* each key NULL in turn: its field stays 0, it reads back 0, and
         * the others are untouched */
        for (int nk = 0; nk < c.n && round < 50; nk++) {
            uint64_t n0 = 0, n1 = 0;
            const uint32_t flag = 0x80u >> nk;
            for (int k = 0; k < c.n; k++)
                if (k != nk) bk_key_put(&l, k, e[k], &n0, &n1);
            for (int k = 0; k < c.n; k++) {
                const uint64_t g = bk_key_get(&l, k, n0, n1, flag);
                CHECK(g == (k == nk ? 0 : e[k]), "%s: NULL key %d, key %d got %llx",
                      c.name, nk, k, (unsigned long long)g);
            }
        }
    }
}

static uint64_t dbits(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}

struct Fin {
    int at;
    int32_t vt;
    uint64_t val, cnt;
    int has;
    uint64_t bits;
    int32_t out_type;
    int count_shaped;
};

static void check_finalize() {
    const uint64_t M5 = (uint64_t)(int64_t)-5, M3 = (uint64_t)(int64_t)-3;
    const Fin F[] = {
        /* COUNT-shaped: the value word, never NULL, INT64 whatever the input */
        {BK_AGG_COUNT_STAR, BK_INT64, 7, 0, 1, 7, BK_INT64, 1},
        {BK_AGG_COUNT_STAR, BK_DOUBLE, 0, 0, 1, 0, BK_INT64, 1},
        {BK_AGG_COUNT, BK_INT64, 3, 0, 1, 3, BK_INT64, 1},
        {BK_AGG_COUNT, BK_DOUBLE, 4, 0, 1, 4, BK_INT64, 1},
        {BK_AGG_COUNT, BK_STRING, 0, 0, 1, 0, BK_INT64, 1},
        {BK_AGG_COUNT_DISTINCT, BK_INT64, 11, 0, 1, 11, BK_INT64, 1},
        {BK_AGG_COUNT_DISTINCT, BK_STRING, 2, 0, 1, 2, BK_INT64, 1},
        /* SUM keeps the input type; NULL over no input */
        {BK_AGG_SUM, BK_INT64, M5, 2, 1, M5, BK_INT64, 0},
        {BK_AGG_SUM, BK_INT64, 0, 0, 0, 0, BK_INT64, 0},
        {BK_AGG_SUM, BK_DOUBLE, 0x4004000000000000ull /* 2.5 */, 3, 1,
         0x4004000000000000ull, BK_DOUBLE, 0},
        {BK_AGG_SUM, BK_DOUBLE, 0, 0, 0, 0, BK_DOUBLE, 0},
        {BK_AGG_SUM_DISTINCT, BK_INT64, 40, 4, 1, 40, BK_INT64, 0},
        {BK_AGG_SUM_DISTINCT, BK_DOUBLE, 0x3FF8000000000000ull /* 1.5 */, 1,
         1, 0x3FF8000000000000ull, BK_DOUBLE, 0},
        {BK_AGG_SUM_DISTINCT, BK_INT64, 0, 0, 0, 0, BK_INT64, 0},
        /* AVG: f64 sum / count, DOUBLE whatever the input. 7.0 / 2 = 3.5 */
        {BK_AGG_AVG, BK_INT64, 0x401C000000000000ull, 2, 1,
         0x400C000000000000ull, BK_DOUBLE, 0},
        {BK_AGG_AVG, BK_DOUBLE, 0x401C000000000000ull, 2, 1,
         0x400C000000000000ull, BK_DOUBLE, 0},
        /* 1.0 / 3 rounds to 0x3FD5555555555555 */
        {BK_AGG_AVG, BK_DOUBLE, 0x3FF0000000000000ull, 3, 1,
         0x3FD5555555555555ull, BK_DOUBLE, 0},
        {BK_AGG_AVG, BK_INT64, 0, 0, 0, 0, BK_DOUBLE, 0},
        {BK_AGG_AVG_DISTINCT, BK_INT64, 0x401C000000000000ull, 2, 1,
         0x400C000000000000ull, BK_DOUBLE, 0},
        {BK_AGG_AVG_DISTINCT, BK_DOUBLE, 0, 0, 0, 0, BK_DOUBLE, 0},
        /* MIN keeps ~enc, MAX keeps enc. INT64 -3: enc 0x7FFF...FD */
        {BK_AGG_MIN, BK_INT64, 0x8000000000000002ull, 1, 1, M3, BK_INT64, 0},
        {BK_AGG_MAX, BK_INT64, 0x8000000000000009ull, 5, 1, 9, BK_INT64, 0},
        {BK_AGG_MIN, BK_INT64, 0, 0, 0, 0, BK_INT64, 0},
        {BK_AGG_MAX, BK_INT64, 0, 0, 0, 0, BK_INT64, 0},
        /* DOUBLE -1.5 = 0xBFF8...: negative, enc = ~bits, state = ~enc */
        {BK_AGG_MIN, BK_DOUBLE, 0xBFF8000000000000ull, 2, 1,
         0xBFF8000000000000ull, BK_DOUBLE, 0},
        /* DOUBLE 2.0 = 0x4000...: enc sets the sign bit */
        {BK_AGG_MAX, BK_DOUBLE, 0xC000000000000000ull, 2, 1,
         0x4000000000000000ull, BK_DOUBLE, 0},
        {BK_AGG_MIN, BK_DOUBLE, 0, 0, 0, 0, BK_DOUBLE, 0},
        /* STRING code 17: enc is the code */
        {BK_AGG_MIN, BK_STRING, 0xFFFFFFFFFFFFFFEEull, 1, 1, 17, BK_STRING, 0},
        {BK_AGG_MAX, BK_STRING, 17, 1, 1, 17, BK_STRING, 0},
        {BK_AGG_MAX, BK_STRING, 0, 0, 0, 0, BK_STRING, 0},
    };
    for (const Fin& f : F) {
        uint64_t bits = 0xDEADBEEFull;
        const int has = bk_agg_finalize(f.at, f.vt, f.val, f.cnt, &bits);
        CHECK(has == f.has, "finalize kind %d type %d cnt %llu: has %d", f.at,
              f.vt, (unsigned long long)f.cnt, has);
        CHECK(bits == f.bits, "finalize kind %d type %d cnt %llu: %llx want %llx",
              f.at, f.vt, (unsigned long long)f.cnt, (unsigned long long)bits,
              (unsigned long long)f.bits);
        CHECK(bk_agg_out_type(f.at, f.vt) == f.out_type,
              "out type kind %d type %d", f.at, f.vt);
        CHECK(bk_agg_count_shaped(f.at) == f.count_shaped,
              "count shaped kind %d", f.at);
    }
    /* the hand-written double patterns are what they claim to be */
    CHECK(dbits(2.5) == 0x4004000000000000ull && dbits(7.0) == 0x401C000000000000ull &&
          dbits(3.5) == 0x400C000000000000ull && dbits(-1.5) == 0xBFF8000000000000ull &&
          dbits(2.0) == 0x4000000000000000ull && dbits(1.0 / 3.0) == 0x3FD5555555555555ull,
          "double bit patterns");
}

int main() {
    std::mt19937_64 rng(20240607);
    for (const Case& c : CASES) {
        const BkQuerySpec q = spec_of(c);
        const BkKeyLayout l = bk_key_layout(&q);
        check_walk(c, l);
        check_round_trip(c, l, rng);
    }
    {
        const BkQuerySpec q = spec_of(THREE_WORDS);
        check_walk(THREE_WORDS, bk_key_layout(&q));
    }
    {   /* no GROUP BY: no words */
        static BkQuerySpec q;
        memset(&q, 0, sizeof q);
        CHECK(bk_key_layout(&q).nwords == 0, "n_group 0: nwords");
    }
    check_finalize();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("keylayout ok: %zu layouts\n", sizeof CASES / sizeof CASES[0] + 1);
    return 0;
}
