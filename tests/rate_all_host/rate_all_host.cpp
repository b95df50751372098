// TEST INFRASTRUCTURE: the event limiters' placement rule on the CPU. The rule is the
// product's (siddhi_amd/csrc/sh_rate.h shl_place, what k_shl_rel runs per row); this
// file only reads a job, sorts the rows stably by (query, key), and places them the
// way sh_rate.hip does: release row, weights in row order, their exclusive scan.
//
// Job file (little endian, tests/rate_host's with n_cuts == 0):
//   int32 n_queries, int32 0, int64 m
//   n_queries x (int32 kind, int32 n)
//   int32 query[m], int32 key[m]
// Output: "rows" and the source row of every output row, in output order.
// Exit 1 on a malformed job, 2 when two rows take one place or a place stays empty.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <vector>

#include "../../siddhi_amd/csrc/sh_rate.h"

namespace {
bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: rate_all_host JOB\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t hdr[2];
    int64_t m;
    if (!rd(f, hdr, 8) || !rd(f, &m, 8)) return 1;
    const int32_t nq = hdr[0];
    if (nq < 1 || nq > 4096 || hdr[1] != 0 || m < 0 || m > (1ll << 28)) return 1;
    std::vector<shl_rule> rules((size_t)nq);
    std::vector<int32_t> query((size_t)m), key((size_t)m);
    if (!rd(f, rules.data(), rules.size() * sizeof(shl_rule)) || !rd(f, query.data(), query.size() * 4) ||
        !rd(f, key.data(), key.size() * 4))
        return 1;
    fclose(f);
    for (int64_t r = 0; r < m; r++)
        if (query[(size_t)r] < 0 || query[(size_t)r] >= nq) return 1;
    auto run_key = [&](int64_t r) { return ((uint64_t)(uint32_t)query[(size_t)r] << 32) | (uint32_t)key[(size_t)r]; };
    std::vector<int64_t> idx((size_t)m);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return run_key(a) < run_key(b); });
    const int64_t none = -1;
    std::vector<int64_t> rel((size_t)m, none), choff((size_t)m, 0), wgt((size_t)m, 0), woff((size_t)m, 0);
    int64_t head = 0;
    for (int64_t p = 0; p < m; p++) {
        const int64_t r = idx[(size_t)p];
        if (p == 0 || run_key(idx[(size_t)(p - 1)]) != run_key(r)) head = p;
        const shl_spot S = shl_place(rules[(size_t)query[(size_t)r]], (uint64_t)(p - head) + 1);
        const int64_t pr = p + (int64_t)S.ahead;
        if (S.leaves && pr < m && run_key(idx[(size_t)pr]) == run_key(r)) rel[(size_t)r] = idx[(size_t)pr];
        choff[(size_t)r] = S.offset;
        wgt[(size_t)r] = S.weight;
    }
    int64_t total = 0;
    for (int64_t r = 0; r < m; r++) {
        woff[(size_t)r] = total;
        total += wgt[(size_t)r];
    }
    if (total > m) return 2;
    std::vector<int64_t> src_of((size_t)total, none);
    for (int64_t r = 0; r < m; r++) {
        if (rel[(size_t)r] == none) continue;
        const int64_t d = woff[(size_t)rel[(size_t)r]] + choff[(size_t)r];
        if (d < 0 || d >= total || src_of[(size_t)d] != none) return 2;
        src_of[(size_t)d] = r;
    }
    printf("rows");
    for (int64_t d = 0; d < total; d++) {
        if (src_of[(size_t)d] == none) return 2;
        printf(" %lld", (long long)src_of[(size_t)d]);
    }
    printf("\n");
    return 0;
}
