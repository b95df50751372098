// TEST INFRASTRUCTURE: the output-row `having` predicate on the CPU. The lowering
// and the evaluation are the product's (siddhi_amd/csrc/sh_having.h, what
// k_shv_mark runs per row); this file only reads a job and prints the keep mask.
//
// Job file (little endian):
//   int32 n_queries, int32 n_out (row stride), int64 m, int32 has_nulls, int32 pad
//   per query: int32 n_outputs, int32 n_exprs, int32 having, int32 pad,
//              n_outputs x sh_output_attr, n_exprs x sh_expr
//   int32 query[m], int64 vals[m * n_out], uint8 nulls[m * n_out] (when has_nulls)
// Output: one line per query, "q <id> <instructions, -1: not lowerable>", then
// "mask " and one character per row, 1 kept / 0 dropped. Exit 2 when a query with a
// `having` does not lower (no mask is printed), 1 on a malformed job.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../siddhi_amd/csrc/sh_having.h"

namespace {
bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: having_host JOB\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t hdr[2];
    int64_t m;
    int32_t tail[2];
    if (!rd(f, hdr, 8) || !rd(f, &m, 8) || !rd(f, tail, 8)) return 1;
    const int32_t nq = hdr[0], n_out = hdr[1];
    if (nq < 1 || nq > 4096 || n_out < 1 || n_out > SHV_MAX_OUT || m < 0 || m > (1ll << 28)) return 1;
    std::vector<shv_prog> progs(nq);
    bool all = true;
    for (int32_t q = 0; q < nq; q++) {
        int32_t qh[4];
        if (!rd(f, qh, 16) || qh[0] < 0 || qh[0] > 64 || qh[1] < 0 || qh[1] > 65536) return 1;
        std::vector<sh_output_attr> outs(qh[0]);
        std::vector<sh_expr> exprs(qh[1]);
        if (!rd(f, outs.data(), outs.size() * sizeof(sh_output_attr)) ||
            !rd(f, exprs.data(), exprs.size() * sizeof(sh_expr)))
            return 1;
        sh_query_desc d;
        memset(&d, 0, sizeof(d));
        d.n_outputs = qh[0];
        d.n_exprs = qh[1];
        d.having = qh[2];
        d.outputs = outs.data();
        d.exprs = exprs.data();
        const int rc = shv_lower(&d, &progs[q]);
        printf("q %d %d\n", q, rc ? -1 : progs[q].n);
        all = all && rc == 0;
    }
    if (!all) return 2;
    std::vector<int32_t> query((size_t)m);
    std::vector<int64_t> vals((size_t)m * n_out);
    std::vector<uint8_t> nulls(tail[0] ? (size_t)m * n_out : 0);
    if (!rd(f, query.data(), query.size() * 4) || !rd(f, vals.data(), vals.size() * 8) ||
        !rd(f, nulls.data(), nulls.size()))
        return 1;
    fclose(f);
    std::string mask((size_t)m, '0');
    for (int64_t r = 0; r < m; r++) {
        const int32_t q = query[r];
        if (q < 0 || q >= nq) return 1;
        if (shv_keep(&progs[q], &vals[(size_t)r * n_out], tail[0] ? &nulls[(size_t)r * n_out] : nullptr)) mask[r] = '1';
    }
    printf("mask %s\n", mask.c_str());
    return 0;
}
