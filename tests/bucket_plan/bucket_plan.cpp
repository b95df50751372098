// TEST INFRASTRUCTURE: run_bucket's select plan and aggregate-carry plan
// (siddhi_amd/csrc/sh_bucket_plan.h) on programs filled in by hand, printed as lines
// of text that tests/test_bucket_plan_cpu.py compares with its expectations.
// Stream attributes are named by index; column pointers are the attribute's index
// into one array, so a printed column is its attribute.
#include <cstdio>
#include <string>
#include <vector>

#include "../../siddhi_amd/csrc/sh_bucket_plan.h"

struct Out {
    int slot, attr, agg;  // e1 = slot 0, e2 = slot 1; an aggregate's argument
};
static const Out COUNT = {1, 0, SH_AGG_COUNT};  // as the lowering writes count()

static const char* tname(int t) {
    static const char* n[] = {"string", "int", "long", "float", "double", "bool", "object"};
    return n[t];
}
static const char* aname(int a) {
    static const char* n[] = {"none", "sum", "avg", "count", "max", "min"};
    return n[a];
}
static std::string list(const int* v, int n) {
    std::string s;
    for (int i = 0; i < n; i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s.empty() ? "-" : s;
}

static char base[32];
static const void* cols[32];

// types: the stream's attributes (0: the partition attribute); staged: the attributes
// the matcher stages, in its order
static void run(const char* name, std::vector<int> types, std::vector<Out> outs, std::vector<int> staged = {1}) {
    static shp_program P;
    P = shp_program{};
    P.stream_nattr[0] = (int)types.size();
    for (size_t a = 0; a < types.size(); a++) P.attr_type[0][a] = types[a];
    P.n_out = (int)outs.size();
    for (size_t o = 0; o < outs.size(); o++) {
        P.out_slot[o] = outs[o].slot;
        P.out_attr[o] = outs[o].attr;
        P.out_agg[o] = outs[o].agg;
        if (outs[o].agg != SH_AGG_NONE) P.agg_post = 1;
    }
    shb_out O;
    shb_select S;
    if (shb_plan_select(P, 0, cols, &O, &S)) {
        printf("%s select=na\n", name);
        return;
    }
    for (int o = 0; o < P.n_out; o++)
        if ((O.kind[o] == 1) != (S.ms_of[o] < 0) || (O.kind[o] == 1 && O.src[o] != cols[P.out_attr[o]]) ||
            O.type[o] != types[P.out_attr[o]])
            printf("%s select value %d inconsistent\n", name, o);
    printf("%s select=ok ms=%s kind=%s ms_of=%s\n", name, list(S.ms, S.n_ms).c_str(), list(O.kind, P.n_out).c_str(),
           list(S.ms_of, P.n_out).c_str());
    if (!P.agg_post) return;
    shb_plan B{};
    B.n_staged = (int)staged.size();
    for (size_t k = 0; k < staged.size(); k++) {
        B.st_src[k] = cols[staged[k]];
        B.st_width[k] = type_width(types[staged[k]]);
    }
    shb_aggc AG;
    int agg_of[SHB_MAX_OUT];
    const shb_carry_plan cp = shb_plan_carry(P, cols, S.ms_of, &B, &AG, agg_of);
    int st[SHB_MAX_STAGED], sw[SHB_MAX_STAGED];
    for (int k = 0; k < B.n_staged; k++) {
        st[k] = (int)((const char*)B.st_src[k] - base);
        sw[k] = B.st_width[k];
    }
    printf("%s carry=%s staged=%s widths=%s", name, cp == SHB_CARRY ? "carry" : cp == SHB_CARRY_NA ? "na" : "none",
           list(st, B.n_staged).c_str(), list(sw, B.n_staged).c_str());
    if (cp == SHB_CARRY) {
        printf(" n=%d kind=", AG.n);
        for (int i = 0; i < AG.n; i++) printf("%s%s", i ? "," : "", aname(AG.kind[i]));
        printf(" side=%s e1=%d", list(AG.side, AG.n).c_str(), AG.e1_col);
        if (AG.e1_col >= 0) printf(":%s", tname(AG.e1_type));
        for (int c = 0; c < 2; c++) {
            printf(" e2[%d]=%d", c, AG.e2_col[c]);
            if (AG.e2_col[c] >= 0) printf(":%s", tname(AG.e2_type[c]));
        }
        printf(" agg_of=%s", list(agg_of, P.n_out).c_str());
    }
    printf("\n");
}

int main() {
    for (int a = 0; a < 32; a++) cols[a] = base + a;
    const int S = SH_T_STRING, I = SH_T_INT, L = SH_T_LONG, F = SH_T_FLOAT, D = SH_T_DOUBLE, Bo = SH_T_BOOL;
    const int NONE = SH_AGG_NONE, SUM = SH_AGG_SUM, AVG = SH_AGG_AVG;
    // e1.symbol, sum(e2.price), avg(e1.price), count(), sum(e2.volume)
    const std::vector<Out> c2_agg = {{0, 0, NONE}, {1, 1, SUM}, {0, 1, AVG}, COUNT, {1, 2, SUM}};
    run("c2_agg", {S, F, L}, c2_agg);
    run("c2_agg_double", {S, D, L}, c2_agg);
    run("two_8byte_e2", {S, F, L, L}, {{1, 2, SUM}, {1, 3, SUM}});
    run("two_4byte_e1", {S, F, L, I}, {{0, 1, SUM}, {0, 3, SUM}});
    run("same_e1_twice", {S, F, L}, {{0, 1, SUM}, {0, 1, AVG}});
    run("five_aggregates", {S, F, L}, {COUNT, COUNT, COUNT, COUNT, COUNT});
    run("bool_argument", {S, F, L, Bo}, {{1, 3, SUM}});
    run("count_alone", {S, F, L}, {COUNT});
    run("staged_full", {S, F, L, I, F, L}, {{1, 5, SUM}}, {1, 2, 3, 4});
    run("staged_full_among", {S, F, L, I, F, L}, {{1, 3, SUM}}, {1, 2, 3, 4});
    run("five_e1_values", {S, F, L, I, F, L},
        {{0, 1, NONE}, {0, 2, NONE}, {0, 3, NONE}, {0, 4, NONE}, {0, 5, NONE}});
    run("float_partition", {F, F, L}, {{0, 0, NONE}, {1, 1, NONE}});
    return 0;
}
