// sh_bucket_plan.h -- what run_bucket (sh_host_fast.cpp) settles before it allocates
// or launches: where every select value comes from, and whether the carry kernels
// can form the select's aggregates. Arithmetic on the program alone: no HIP call and
// no handle, so a plain C++ compiler takes it (tests/bucket_plan).
#pragma once

#include "../../include/sh_query.h"
#include "sh_device.h"

namespace shh {
inline int type_width(int t) { return t == SH_T_LONG || t == SH_T_DOUBLE ? 8 : (t == SH_T_BOOL ? 1 : 4); }
}  // namespace shh
using shh::type_width;

// select list: e2-side values (and e1's partition attribute, equal to e2's for
// these types) from the consumer row, O->kind 1 with the attribute's column in
// O->src; other e1-side values ride the match stream, O->kind 0 and column
// ms_of[o] of the n_ms attributes ms[] (O->src: the caller's, once allocated).
// 0, or 1 = not applicable (a fifth match-stream column)
struct shb_select {
    int ms[SHB_MAX_MS], n_ms;
    int ms_of[SHB_MAX_OUT];  // -1: a consumer column
};
inline int shb_plan_select(const shp_program& P, int part_attr, const void* const* cols, shb_out* O, shb_select* S) {
    *O = shb_out{};
    O->n_out = P.n_out;
    S->n_ms = 0;
    for (int o = 0; o < P.n_out; o++) {
        const int a = P.out_attr[o], t = P.attr_type[0][a];
        O->type[o] = t;
        S->ms_of[o] = -1;
        const bool fold = a == part_attr && (t == SH_T_STRING || t == SH_T_INT || t == SH_T_LONG || t == SH_T_BOOL);
        if (P.out_slot[o] == 1 || fold) {
            O->kind[o] = 1;
            O->src[o] = cols[a];
            continue;
        }
        int m = 0;
        while (m < S->n_ms && S->ms[m] != a) m++;
        if (m == S->n_ms) {
            if (S->n_ms == SHB_MAX_MS) return 1;
            S->ms[S->n_ms++] = a;
        }
        O->kind[o] = 0;
        S->ms_of[o] = m;
    }
    return 0;
}

// aggregators carried per key (k_bk_aggp / k_bk_aggc): e1-side arguments from one
// 4-byte match-stream column, e2-side ones from up to two staged columns (one of
// them 4-byte), count() without one; anything else leaves the arguments in the rows
// for the post-pass (sh_agg.hip). B->st_src / st_width / n_staged hold the matcher's
// staged columns on entry and gain the e2 arguments' (the consumer's column at its
// slot: the matcher's own first, then the carry's; st_dst is the caller's, once
// allocated). agg_of[o]: select value o's aggregate in AG, -1 none. SHB_CARRY: AG holds
// the carry; _NA: the staged columns are full, the engine is not applicable; _NONE:
// not a carried form, the rows carry the arguments
enum shb_carry_plan { SHB_CARRY = 0, SHB_CARRY_NA = 1, SHB_CARRY_NONE = 2 };
inline shb_carry_plan shb_plan_carry(const shp_program& P, const void* const* cols, const int* ms_of, shb_plan* B,
                                     shb_aggc* AG, int* agg_of) {
    *AG = shb_aggc{};
    AG->e1_col = AG->e2_col[0] = AG->e2_col[1] = -1;
    for (int o = 0; o < P.n_out; o++) agg_of[o] = -1;
    for (int o = 0; o < P.n_out; o++) {
        const int ak = P.out_agg[o];
        if (ak == SH_AGG_NONE) continue;
        if (AG->n == SHB_MAX_AGG || (ak != SH_AGG_SUM && ak != SH_AGG_AVG && ak != SH_AGG_COUNT)) return SHB_CARRY_NONE;
        const int i = AG->n++;
        AG->kind[i] = ak;
        agg_of[o] = i;
        if (ak == SH_AGG_COUNT) {
            AG->side[i] = 3;
            continue;
        }
        const int a = P.out_attr[o], t = P.attr_type[0][a];
        if (t != SH_T_INT && t != SH_T_FLOAT && t != SH_T_LONG && t != SH_T_DOUBLE) return SHB_CARRY_NONE;
        const int w = type_width(t);
        if (P.out_slot[o] == 0 && ms_of[o] >= 0 && w == 4 && (AG->e1_col < 0 || AG->e1_col == ms_of[o])) {
            AG->e1_col = ms_of[o];
            AG->e1_type = t;
            AG->side[i] = 0;
        } else if (P.out_slot[o] == 1) {
            int k = 0;
            while (k < B->n_staged && B->st_src[k] != cols[a]) k++;
            if (k == B->n_staged) {
                if (B->n_staged == SHB_MAX_STAGED) return SHB_CARRY_NA;
                B->st_src[k] = cols[a];
                B->st_width[k] = w;
                B->n_staged++;
            }
            int c = (AG->e2_col[0] == k) ? 0 : (AG->e2_col[1] == k ? 1 : -1);
            if (c < 0) {
                if (AG->e2_col[0] < 0) c = 0;
                else if (AG->e2_col[1] < 0 && w == 4) c = 1;
                else if (AG->e2_col[1] < 0 && type_width(AG->e2_type[0]) == 4) {
                    // keep the 8-byte column in slot 0
                    AG->e2_col[1] = AG->e2_col[0];
                    AG->e2_type[1] = AG->e2_type[0];
                    for (int j = 0; j < i; j++)
                        if (AG->side[j] == 1) AG->side[j] = 2;
                    c = 0;
                } else {
                    return SHB_CARRY_NONE;
                }
                AG->e2_col[c] = k;
                AG->e2_type[c] = t;
            }
            AG->side[i] = 1 + c;
        } else {
            return SHB_CARRY_NONE;
        }
    }
    return SHB_CARRY;
}
