// bk_keylayout.h — the two rules every reader of an aggregate result needs,
// each stated once for host C++ and device code:
//   1. where group key k sits in the two packed 64-bit key words
//      (BkQuerySpec.group_bits/group_base, bk_common.h), and
//   2. how a finished aggregate state {val, cnt} becomes an output value,
//      and of what type (agg_fn_call.cpp:927-975).
// NOT included by oracle/: the oracle is the independent check of both.
#ifndef BK_KEYLAYOUT_H
#define BK_KEYLAYOUT_H

#include "bk_common.h"
#include "bk_keyenc.h"

/* Position of every group key: sequential shift packing, a key that does not
 * fit the current word starts the next one (keys never straddle words).
 * bits is the declared width, or 64 for an undeclared (full-word) key;
 * base_enc is the encoding of the declared base (STRING codes raw, otherwise
 * bk_enc_i64), 0 for a full-word key, so field + base_enc is always the
 * key's full order-preserving encoding.
 * The row path packs with its own in-register copy of this walk,
 * pack_group_keys (bkgpu.hip): change the two together. */
typedef struct BkKeyLayout {
    int32_t  n;
    int32_t  bits[BK_MAX_GROUP];
    int32_t  shift[BK_MAX_GROUP];
    int32_t  word[BK_MAX_GROUP];
    uint64_t base_enc[BK_MAX_GROUP];
    int32_t  nwords;    /* 64-bit words occupied; the engine holds two */
} BkKeyLayout;

/* n_group beyond BK_MAX_GROUP is clamped (the spec's arrays end there; the
 * entry points refuse such a spec before any key is read) */
BK_KHD BkKeyLayout bk_key_layout(const BkQuerySpec* q) {
    BkKeyLayout l;
    memset(&l, 0, sizeof l);
    l.n = q->n_group < BK_MAX_GROUP ? q->n_group : BK_MAX_GROUP;
    int shift = 0, word = 0;
    for (int k = 0; k < l.n; k++) {
        int bits = q->group_bits[k] ? q->group_bits[k] : 64;
        if (shift + bits > 64) { word++; shift = 0; }
        l.bits[k] = bits;
        l.shift[k] = shift;
        l.word[k] = word;
        if (bits < 64)
            l.base_enc[k] = q->group_types[k] == BK_STRING
                                ? (uint64_t)q->group_base[k]
                                : bk_enc_i64(q->group_base[k]);
        shift += bits;
    }
    l.nwords = l.n > 0 ? word + 1 : 0;
    return l;
}

/* low `bits` ones, bits in 1..64 (never a shift by 64). bits == 0, the
 * value of an unused slot k >= n, is NOT allowed: bk_key_get and bk_key_put
 * require 0 <= k < n. */
BK_KHD uint64_t bk_key_mask(int32_t bits) { return ~0ull >> (64 - bits); }

/* full encoding of key k; 0 for a NULL key (null bit: flag >> (7-k),
 * exec_node.cpp:561) */
BK_KHD uint64_t bk_key_get(const BkKeyLayout* l, int k, uint64_t k0,
                           uint64_t k1, uint32_t flag) {
    if ((flag >> (7 - k)) & 1) return 0;
    const uint64_t w = l->word[k] == 0 ? k0 : k1;
    return ((w >> l->shift[k]) & bk_key_mask(l->bits[k])) + l->base_enc[k];
}

/* inverse of bk_key_get for a non-NULL key (a NULL key's field stays 0) */
BK_KHD void bk_key_put(const BkKeyLayout* l, int k, uint64_t enc,
                       uint64_t* k0, uint64_t* k1) {
    const uint64_t f = ((enc - l->base_enc[k]) & bk_key_mask(l->bits[k]))
                       << l->shift[k];
    if (l->word[k] == 0) *k0 |= f; else *k1 |= f;
}

/* COUNT-shaped aggregates: the state's value word is the result, never NULL */
BK_KHD int bk_agg_count_shaped(int agg_type) {
    return agg_type == BK_AGG_COUNT_STAR || agg_type == BK_AGG_COUNT ||
           agg_type == BK_AGG_COUNT_DISTINCT;
}

/* output type of an aggregate (agg_fn_call.cpp:96-99, 927-975) */
BK_KHD int32_t bk_agg_out_type(int agg_type, int32_t in_type) {
    if (bk_agg_count_shaped(agg_type)) return BK_INT64;
    if (agg_type == BK_AGG_AVG || agg_type == BK_AGG_AVG_DISTINCT)
        return BK_DOUBLE;
    return in_type;     /* SUM/MIN/MAX keep the input type */
}

/* decode an order-preserving encoding into the 64 bits of a cell of `type`:
 * double bits, a STRING code, or an int64 */
BK_KHD uint64_t bk_enc_to_cell(int32_t type, uint64_t e) {
    if (type == BK_DOUBLE) {
        double d = bk_dec_f64(e);
        uint64_t u;
        memcpy(&u, &d, 8);
        return u;
    }
    if (type == BK_STRING) return (uint64_t)(uint32_t)e;
    return (uint64_t)bk_dec_i64(e);
}

/* finished state {val, cnt} -> output cell of bk_agg_out_type(), as 64 raw
 * bits in *bits64 (0 when NULL). Returns whether the result is non-NULL. */
BK_KHD int bk_agg_finalize(int agg_type, int32_t in_type, uint64_t val,
                           uint64_t cnt, uint64_t* bits64) {
    *bits64 = 0;
    switch (agg_type) {
        case BK_AGG_COUNT_STAR:
        case BK_AGG_COUNT:
        case BK_AGG_COUNT_DISTINCT:
            *bits64 = val;
            return 1;
        case BK_AGG_SUM:
        case BK_AGG_SUM_DISTINCT:
            if (!cnt) return 0;
            *bits64 = val;
            return 1;
        case BK_AGG_AVG:
        case BK_AGG_AVG_DISTINCT: {
            if (!cnt) return 0;
            double s;
            memcpy(&s, &val, 8);
            double q = s / (double)cnt;   /* the one IEEE f64 division */
            memcpy(bits64, &q, 8);
            return 1;
        }
        case BK_AGG_MIN:    /* MIN keeps the complement, so both are a max */
        case BK_AGG_MAX:
            if (!cnt) return 0;
            *bits64 = bk_enc_to_cell(in_type,
                                     agg_type == BK_AGG_MIN ? ~val : val);
            return 1;
        default:
            return 0;
    }
}

#endif /* BK_KEYLAYOUT_H */
