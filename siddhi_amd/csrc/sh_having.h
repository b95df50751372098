// sh_having.h — an output-only `having` as a predicate over one finished output
// row, as host + device code: sh_having.hip evaluates it one lane per row
// (k_shv_mark), and tests/having_host compiles the same code for the CPU.
//
// The reference evaluates `having` after the output attributes and aggregators of
// the row are set (QuerySelector.java:161-205, 271-313), and a state query's
// selector sees one state event per chunk, so a condition that reads only output
// attributes (SH_OP_OUTPUT) and constants is a pure function of the row: an ordered
// row filter behind any engine, with no state between steps.
//
// shv_lower turns sh_query_desc.having into a postfix program of at most
// SHV_MAX_CODE instructions whose stack never exceeds SHV_MAX_STACK; operand types
// are static, so an instruction carries them and the stack holds raw 8-byte values
// and one null bit each. The stack is a shift register (s[0] is the top, every
// index a constant), so it lives in registers on the device: no scratch.
// Semantics are the general engine's (sh_nfa.h eval / having_ok) through the same
// helpers (sh_nfa_val.h nf_cmp / nf_arith): null propagates through arithmetic, x/0
// and x%0 are null, a compare with null is false, not(null) is true, and the row
// passes only when the condition is non-null and true.
#pragma once
#include <stdint.h>

#include "../../include/sh_query.h"
#include "sh_nfa_val.h"

#define SHV_MAX_CODE 32
#define SHV_MAX_STACK 8
#define SHV_MAX_CONST 16
#define SHV_MAX_OUT 16

// opcodes are shp_opcode's (sh_program.h); the fields a postfix step needs
struct shv_instr {
    uint8_t op;   // OPC_CONST, OPC_OUTPUT, OPC_AND, OPC_OR, OPC_NOT, OPC_BOOLV, OPC_CMP, OPC_ARITH, OPC_ISNULL, OPC_SELECT
    uint8_t a;    // CMP / ARITH: the sh_op; CONST: the constant is null
    uint8_t b;    // CMP: domain; ARITH: result type
    uint8_t lt;   // CMP / ARITH: left operand type; CONST / OUTPUT: the value's type
    uint8_t rt;   // CMP / ARITH: right operand type
    uint8_t x;    // CONST: constant index; OUTPUT: output attribute
    uint8_t pad[2];
};

// one query's program; n == 0 keeps every row
struct shv_prog {
    int32_t n;
    int32_t n_const;
    shv_instr code[SHV_MAX_CODE];
    int64_t consts[SHV_MAX_CONST];
};

struct shv_stack {
    int64_t s[SHV_MAX_STACK];
    uint32_t nw;  // bit d: the value at depth d is null
    NF_INL void push(int64_t v, uint32_t isnull) {
#pragma unroll
        for (int i = SHV_MAX_STACK - 1; i > 0; i--) s[i] = s[i - 1];
        s[0] = v;
        nw = (nw << 1) | (isnull ? 1u : 0u);
    }
    NF_INL NfVal pop(int type) {
        NfVal v;
        v.b = s[0];
        v.t = (uint8_t)type;
        v.null = (uint8_t)(nw & 1u);
#pragma unroll
        for (int i = 0; i + 1 < SHV_MAX_STACK; i++) s[i] = s[i + 1];
        nw >>= 1;
        return v;
    }
};

// the row passes: `row` its n_out raw values, `nulls` its null flags or NULL
NF_INL bool shv_keep(const shv_prog* P, const int64_t* row, const uint8_t* nulls) {
    const int n = P->n;
    if (n <= 0) return true;
    shv_stack S;
#pragma unroll
    for (int i = 0; i < SHV_MAX_STACK; i++) S.s[i] = 0;
    S.nw = 0;
    for (int k = 0; k < n && k < SHV_MAX_CODE; k++) {
        const shv_instr in = P->code[k];
        switch (in.op) {
            case OPC_CONST: S.push(P->consts[in.x & (SHV_MAX_CONST - 1)], in.a); break;
            case OPC_OUTPUT: {
                const int o = in.x & (SHV_MAX_OUT - 1);
                S.push(row[o], nulls ? nulls[o] : 0u);
                break;
            }
            case OPC_AND: {
                const NfVal r = S.pop(SH_T_BOOL), l = S.pop(SH_T_BOOL);
                S.push((!l.null && l.b && !r.null && r.b) ? 1 : 0, 0);
                break;
            }
            case OPC_OR: {
                const NfVal r = S.pop(SH_T_BOOL), l = S.pop(SH_T_BOOL);
                S.push(((!l.null && l.b) || (!r.null && r.b)) ? 1 : 0, 0);
                break;
            }
            case OPC_NOT: {
                const NfVal l = S.pop(SH_T_BOOL);
                S.push((!l.null && l.b) ? 0 : 1, 0);  // Not(null) = true
                break;
            }
            case OPC_BOOLV: {
                const NfVal l = S.pop(SH_T_BOOL);
                S.push((!l.null && l.b) ? 1 : 0, 0);
                break;
            }
            case OPC_ISNULL: {
                const NfVal l = S.pop(in.lt);
                S.push(l.null ? 1 : 0, 0);
                break;
            }
            case OPC_CMP: {
                const NfVal r = S.pop(in.rt), l = S.pop(in.lt);
                S.push((!l.null && !r.null && nf_cmp(in.a, in.b, l, r)) ? 1 : 0, 0);
                break;
            }
            case OPC_ARITH: {
                const NfVal r = S.pop(in.rt), l = S.pop(in.lt);
                const NfVal o = nf_arith(in.a, in.b, l, r);
                S.push(o.b, o.null);
                break;
            }
            case OPC_SELECT: {  // if-then-else: the chosen operand's bits, retagged by its consumer
                const NfVal e = S.pop(in.lt), t = S.pop(in.lt), c = S.pop(SH_T_BOOL);
                const NfVal& o = (!c.null && c.b) ? t : e;
                S.push(o.b, o.null);
                break;
            }
            default: break;
        }
    }
    const NfVal v = S.pop(SH_T_BOOL);
    return !v.null && v.b;
}

// ---- lowering (host): 0 lowered into *P (q->having < 0: the empty program), 1 not
// lowerable -- a state-event attribute (SH_OP_VAR), IS_NULL_STREAM, a List or object
// operand, a string compare other than == / !=, or a program beyond the bounds
struct shv_lowering {
    const sh_query_desc* q;
    shv_prog* P;
    int depth, max_depth;
    bool emit(uint8_t op, uint8_t a, uint8_t b, uint8_t lt, uint8_t rt, uint8_t x, int pops) {
        if (P->n >= SHV_MAX_CODE) return false;
        shv_instr& in = P->code[P->n++];
        in.op = op;
        in.a = a;
        in.b = b;
        in.lt = lt;
        in.rt = rt;
        in.x = x;
        in.pad[0] = in.pad[1] = 0;
        depth += 1 - pops;
        if (depth > max_depth) max_depth = depth;
        return depth <= SHV_MAX_STACK;
    }
    static bool plain(int t) { return t >= SH_T_STRING && t <= SH_T_BOOL; }
    static int dom_for(int op, int lt, int rt) {
        if (lt == SH_T_STRING || rt == SH_T_STRING) return DOM_STR;
        if (lt == SH_T_BOOL || rt == SH_T_BOOL) return DOM_BOOL;
        const int rl = lt == SH_T_INT ? 0 : lt == SH_T_LONG ? 1 : lt == SH_T_FLOAT ? 2 : 3;
        const int rr = rt == SH_T_INT ? 0 : rt == SH_T_LONG ? 1 : rt == SH_T_FLOAT ? 2 : 3;
        int r = rl > rr ? rl : rr;
        // Equal / NotEqual FloatLong and LongFloat compare as double
        const bool fl = (lt == SH_T_FLOAT && rt == SH_T_LONG) || (lt == SH_T_LONG && rt == SH_T_FLOAT);
        if ((op == SH_OP_EQ || op == SH_OP_NE) && fl) r = 3;
        return r == 0 ? DOM_I32 : r == 1 ? DOM_I64 : r == 2 ? DOM_F32 : DOM_F64;
    }
    bool gen(int e, int rec) {
        if (e < 0 || e >= q->n_exprs || rec > SHV_MAX_CODE) return false;
        const sh_expr& x = q->exprs[e];
        if (!plain(x.type)) return false;
        switch (x.op) {
            case SH_OP_CONST: {
                int c = 0;
                for (; c < P->n_const; c++)
                    if (P->consts[c] == x.cval) break;
                if (c == P->n_const) {
                    if (c >= SHV_MAX_CONST) return false;
                    P->consts[P->n_const++] = x.cval;
                }
                return emit(OPC_CONST, x.is_null ? 1 : 0, 0, (uint8_t)x.type, 0, (uint8_t)c, 0);
            }
            case SH_OP_OUTPUT:
                if (x.attr < 0 || x.attr >= q->n_outputs || x.attr >= SHV_MAX_OUT) return false;
                if (q->outputs[x.attr].type != x.type) return false;
                return emit(OPC_OUTPUT, 0, 0, (uint8_t)x.type, 0, (uint8_t)x.attr, 0);
            case SH_OP_NOT: return gen(x.lhs, rec + 1) && emit(OPC_NOT, 0, 0, 0, 0, 0, 1);
            case SH_OP_BOOL_VAR: return gen(x.lhs, rec + 1) && emit(OPC_BOOLV, 0, 0, 0, 0, 0, 1);
            case SH_OP_IS_NULL:
                return gen(x.lhs, rec + 1) && emit(OPC_ISNULL, 0, 0, (uint8_t)q->exprs[x.lhs].type, 0, 0, 1);
            case SH_OP_AND:
            case SH_OP_OR:
                return gen(x.lhs, rec + 1) && gen(x.rhs, rec + 1) &&
                       emit(x.op == SH_OP_AND ? OPC_AND : OPC_OR, 0, 0, 0, 0, 0, 2);
            case SH_OP_EQ:
            case SH_OP_NE:
            case SH_OP_GT:
            case SH_OP_GE:
            case SH_OP_LT:
            case SH_OP_LE: {
                if (x.lhs < 0 || x.lhs >= q->n_exprs || x.rhs < 0 || x.rhs >= q->n_exprs) return false;
                const int lt = q->exprs[x.lhs].type, rt = q->exprs[x.rhs].type;
                const int dom = dom_for(x.op, lt, rt);
                if (dom == DOM_STR && (lt != rt || (x.op != SH_OP_EQ && x.op != SH_OP_NE))) return false;
                return gen(x.lhs, rec + 1) && gen(x.rhs, rec + 1) &&
                       emit(OPC_CMP, (uint8_t)x.op, (uint8_t)dom, (uint8_t)lt, (uint8_t)rt, 0, 2);
            }
            case SH_OP_ADD:
            case SH_OP_SUB:
            case SH_OP_MUL:
            case SH_OP_DIV:
            case SH_OP_MOD: {
                if (x.lhs < 0 || x.lhs >= q->n_exprs || x.rhs < 0 || x.rhs >= q->n_exprs) return false;
                const int lt = q->exprs[x.lhs].type, rt = q->exprs[x.rhs].type;
                if (x.type < SH_T_INT || x.type > SH_T_DOUBLE) return false;
                return gen(x.lhs, rec + 1) && gen(x.rhs, rec + 1) &&
                       emit(OPC_ARITH, (uint8_t)x.op, (uint8_t)x.type, (uint8_t)lt, (uint8_t)rt, 0, 2);
            }
            case SH_OP_IF_THEN_ELSE:
                return gen(x.lhs, rec + 1) && gen(x.rhs, rec + 1) && gen(x.third, rec + 1) &&
                       emit(OPC_SELECT, 0, 0, (uint8_t)x.type, 0, 0, 3);
            default: return false;  // SH_OP_VAR, IS_NULL_STREAM, MULTI_VAR
        }
    }
};

inline int shv_lower(const sh_query_desc* q, shv_prog* P) {
    __builtin_memset(P, 0, sizeof(*P));
    if (q->having < 0) return 0;
    for (int o = 0; o < q->n_outputs; o++)
        if (q->outputs[o].expr >= 0 && q->outputs[o].expr < q->n_exprs &&
            q->exprs[q->outputs[o].expr].op == SH_OP_MULTI_VAR)
            return 1;
    shv_lowering L{q, P, 0, 0};
    if (!L.gen(q->having, 0) || L.depth != 1 || P->n < 1) {
        __builtin_memset(P, 0, sizeof(*P));
        return 1;
    }
    return 0;
}

// ---- the device filter (sh_having.hip): a stable compaction of ordered rows
#define SHV_TILE 256  // rows per tile: one workgroup, one row per lane in the mark
// A set of m ordered rows as parallel columns, to read and to write: vals holds
// m x n_out raw values and nulls their null flags (NULL: none are null); seq, query,
// ts and key (the row's partition key) hold one entry per row. Only vals is
// mandatory. A pass moves a column iff its destination is set (NULL copies nothing)
// and refuses (-1) a destination whose source column is NULL. The two sets never
// overlap: a workgroup may write a destination another has yet to read.
struct shw_rows {
    const uint64_t* seq; const int64_t* vals; const int32_t* query;
    const int64_t* ts; const uint8_t* nulls; const int32_t* key;
};
struct shw_rows_out {
    uint64_t* seq; int64_t* vals; int32_t* query;
    int64_t* ts; uint8_t* nulls; int32_t* key;
};
#ifdef __cplusplus
extern "C" {
#endif
// 4-byte words of workspace for m rows: the ballot words (2 per 64 rows), the tiles'
// kept counts and their exclusive scan, and the scan's own block sums
int64_t shv_filter_ws_words(int64_t m);
// Keeps row r of the m ordered rows of src iff progs[query[r]] (progs[0] when query is
// NULL; a query id outside [0, n_progs) keeps the row) passes on its values
// vals[r * n_out ..] and null flags nulls[r * n_out ..]. The kept rows go, in order,
// to dst (each column as long as its source). *d_kept (device, 8 bytes) takes the kept
// count. 1 <= n_out <= SHV_MAX_OUT, m < 2^31; ws: shv_filter_ws_words(m) words.
// All launches are asynchronous on `stream`. 0: launched, < 0: bad arguments.
int shv_filter(const struct shv_prog* progs, int32_t n_progs, int64_t m, int32_t n_out, const struct shw_rows* src,
               const struct shw_rows_out* dst, uint32_t* ws, unsigned long long* d_kept, void* stream);
// The same compaction from ready marks (the event limiter's, sh_rate.hip): mask holds
// one 64-bit ballot word per 64 rows (whole tiles of SHV_TILE rows: rows past m are 0),
// cnt the kept rows of every tile; off [tiles] and tmp [shd_scan_tmp_words(tiles)] are
// scratch. The tiles' counts are scanned and the kept rows moved as shv_filter does.
int shv_move_marked(int64_t m, int32_t n_out, const struct shw_rows* src, const struct shw_rows_out* dst,
                    const uint64_t* mask, const uint32_t* cnt, uint32_t* off, uint32_t* tmp,
                    unsigned long long* d_kept, void* stream);
#ifdef __cplusplus
}
#endif
