// sh_nfa_val.h — typed 8-byte values and the reference's compare and math
// executors over them (core/executor/condition/compare/**, core/executor/math/**),
// as __host__ __device__ code: the general engine (sh_nfa.h) and the output-row
// `having` predicate (sh_having.h) evaluate expressions with these, on the device
// and in the CPU builds of tests/nfa_host and tests/having_host.
#pragma once
#include <stdint.h>

#include "../../include/sh_query.h"
#include "sh_program.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NF_HD __host__ __device__
#else
#define NF_HD
#endif
#define NF_INL NF_HD inline

struct NfVal {
    int64_t b;
    uint8_t t;
    uint8_t null;
};

NF_INL float nf_f32(int64_t b) {
    union {
        uint32_t u;
        float f;
    } x;
    x.u = (uint32_t)b;
    return x.f;
}
NF_INL double nf_f64(int64_t b) {
    union {
        int64_t u;
        double f;
    } x;
    x.u = b;
    return x.f;
}
NF_INL int64_t nf_bf32(float f) {
    union {
        uint32_t u;
        float f;
    } x;
    x.f = f;
    return (int64_t)x.u;
}
NF_INL int64_t nf_bf64(double d) {
    union {
        int64_t u;
        double f;
    } x;
    x.f = d;
    return x.u;
}
NF_INL int64_t nf_to_i64(const NfVal& v) { return v.t == SH_T_LONG ? v.b : (int64_t)(int32_t)v.b; }
NF_INL float nf_to_f32(const NfVal& v) {
    switch (v.t) {
        case SH_T_INT: return (float)(int32_t)v.b;
        case SH_T_LONG: return (float)v.b;
        case SH_T_FLOAT: return nf_f32(v.b);
        default: return (float)nf_f64(v.b);
    }
}
NF_INL double nf_to_f64(const NfVal& v) {
    switch (v.t) {
        case SH_T_INT: return (double)(int32_t)v.b;
        case SH_T_LONG: return (double)v.b;
        case SH_T_FLOAT: return (double)nf_f32(v.b);
        default: return nf_f64(v.b);
    }
}
// Integer/Long/Float/Double/Boolean.compareTo for OrderByEventComparator (operands share
// the executor's return type): Float.compare orders -0.0 before 0.0 and NaN last
NF_INL int nf_java_compare(const NfVal& x, const NfVal& y) {
    switch (x.t) {
        case SH_T_FLOAT: {
            const float a = nf_f32(x.b), c = nf_f32(y.b);
            if (a < c) return -1;
            if (a > c) return 1;
            const int32_t ia = a != a ? 0x7fc00000 : (int32_t)nf_bf32(a);
            const int32_t ic = c != c ? 0x7fc00000 : (int32_t)nf_bf32(c);
            return ia == ic ? 0 : (ia < ic ? -1 : 1);
        }
        case SH_T_DOUBLE: {
            const double a = nf_f64(x.b), c = nf_f64(y.b);
            if (a < c) return -1;
            if (a > c) return 1;
            const int64_t ia = a != a ? 0x7ff8000000000000ll : nf_bf64(a);
            const int64_t ic = c != c ? 0x7ff8000000000000ll : nf_bf64(c);
            return ia == ic ? 0 : (ia < ic ? -1 : 1);
        }
        case SH_T_BOOL: return (int)(x.b != 0) - (int)(y.b != 0);
        default: {
            const int64_t a = nf_to_i64(x), c = nf_to_i64(y);
            return a < c ? -1 : (a > c ? 1 : 0);
        }
    }
}
template <typename T>
NF_INL bool nf_cmp_op(int op, T a, T b) {
    switch (op) {
        case SH_OP_EQ: return a == b;
        case SH_OP_NE: return a != b;
        case SH_OP_GT: return a > b;
        case SH_OP_GE: return a >= b;
        case SH_OP_LT: return a < b;
        default: return a <= b;
    }
}
// compare executors: Java binary numeric promotion of the unboxed operands
// (core/executor/condition/compare/**); ==/!= on Float/Long compare as double
NF_INL bool nf_cmp(int op, int dom, const NfVal& l, const NfVal& r) {
    switch (dom) {
        case DOM_I32: return nf_cmp_op<int32_t>(op, (int32_t)l.b, (int32_t)r.b);
        case DOM_I64: return nf_cmp_op<int64_t>(op, nf_to_i64(l), nf_to_i64(r));
        case DOM_F32: return nf_cmp_op<float>(op, nf_to_f32(l), nf_to_f32(r));
        case DOM_F64: return nf_cmp_op<double>(op, nf_to_f64(l), nf_to_f64(r));
        case DOM_BOOL: return nf_cmp_op<int>(op, l.b != 0, r.b != 0);
        default: return nf_cmp_op<int32_t>(op, (int32_t)l.b, (int32_t)r.b);
    }
}
NF_INL float nf_fmodf(float a, float b) { return __builtin_fmodf(a, b); }
NF_INL double nf_fmod(double a, double b) { return __builtin_fmod(a, b); }
// math executors (core/executor/math/**): result type fixed at parse time;
// integral and floating x/0, x%0 yield null; Java int/long wrap-around
NF_INL NfVal nf_arith(int aop, int rt, const NfVal& l, const NfVal& r) {
    NfVal o;
    o.t = (uint8_t)rt;
    o.null = 0;
    o.b = 0;
    if (l.null || r.null) {
        o.null = 1;
    } else if (rt == SH_T_INT) {
        const uint32_t a = (uint32_t)l.b, b = (uint32_t)r.b;
        const int32_t sa = (int32_t)a, sb = (int32_t)b;
        int32_t res = 0;
        switch (aop) {
            case SH_OP_ADD: res = (int32_t)(a + b); break;
            case SH_OP_SUB: res = (int32_t)(a - b); break;
            case SH_OP_MUL: res = (int32_t)(a * b); break;
            case SH_OP_DIV:
                if (sb == 0) o.null = 1;
                else res = (sa == INT32_MIN && sb == -1) ? INT32_MIN : sa / sb;
                break;
            default:
                if (sb == 0) o.null = 1;
                else res = (sb == -1) ? 0 : sa % sb;
        }
        o.b = res;
    } else if (rt == SH_T_LONG) {
        const uint64_t a = (uint64_t)nf_to_i64(l), b = (uint64_t)nf_to_i64(r);
        const int64_t sa = (int64_t)a, sb = (int64_t)b;
        int64_t res = 0;
        switch (aop) {
            case SH_OP_ADD: res = (int64_t)(a + b); break;
            case SH_OP_SUB: res = (int64_t)(a - b); break;
            case SH_OP_MUL: res = (int64_t)(a * b); break;
            case SH_OP_DIV:
                if (sb == 0) o.null = 1;
                else res = (sa == INT64_MIN && sb == -1) ? INT64_MIN : sa / sb;
                break;
            default:
                if (sb == 0) o.null = 1;
                else res = (sb == -1) ? 0 : sa % sb;
        }
        o.b = res;
    } else if (rt == SH_T_FLOAT) {
        const float a = nf_to_f32(l), b = nf_to_f32(r);
        float res = 0.f;
        switch (aop) {
            case SH_OP_ADD: res = a + b; break;
            case SH_OP_SUB: res = a - b; break;
            case SH_OP_MUL: res = a * b; break;
            case SH_OP_DIV:
                if (b == 0.0f) o.null = 1;
                else res = a / b;
                break;
            default:
                if (b == 0.0f) o.null = 1;
                else res = nf_fmodf(a, b);
        }
        o.b = nf_bf32(res);
    } else {
        const double a = nf_to_f64(l), b = nf_to_f64(r);
        double res = 0.0;
        switch (aop) {
            case SH_OP_ADD: res = a + b; break;
            case SH_OP_SUB: res = a - b; break;
            case SH_OP_MUL: res = a * b; break;
            case SH_OP_DIV:
                if (b == 0.0) o.null = 1;
                else res = a / b;
                break;
            default:
                if (b == 0.0) o.null = 1;
                else res = nf_fmod(a, b);
        }
        o.b = nf_bf64(res);
    }
    return o;
}
