// TEST INFRASTRUCTURE: the `group by` segment rule on the CPU. The rule is the product's
// (siddhi_amd/csrc/sh_group.h shg_word / shg_valid, what k_shg_words runs per row); this
// file only reads a job, sorts the rows stably by (query, key, group words) and numbers
// the segments.
//
// Job file (little endian):
//   int32 n_query, int32 n_out, int64 m
//   n_query x sha_group_q
//   int32 query[m], int32 key[m], int64 vals[m * n_out]
// Output: "order" and the row of every sorted position, then "seg" and the dense segment
// id of every sorted position. `group_host --layout` prints the descriptor's sizes.
// Exit 1 on a malformed job.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../siddhi_amd/csrc/sh_group.h"

namespace {
bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--layout")) {
        printf("sha_group_q %zu sha_groups %zu q %zu col %zu type %zu max_group %d max_queries %d tile %d\n",
               sizeof(sha_group_q), sizeof(sha_groups), offsetof(sha_groups, q), offsetof(sha_group_q, col),
               offsetof(sha_group_q, type), SH_MAX_GROUP, SHG_MAX_QUERIES, SHG_TILE);
        return 0;
    }
    if (argc != 2) {
        fprintf(stderr, "usage: group_host JOB | --layout\n");
        return 1;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t hdr[2];
    int64_t m;
    if (!rd(f, hdr, 8) || !rd(f, &m, 8)) return 1;
    const int32_t nq = hdr[0], n_out = hdr[1];
    if (nq < 1 || nq > SHG_MAX_QUERIES || n_out < 1 || n_out > 64 || m < 0 || m > (1ll << 24)) return 1;
    sha_groups G;
    memset(&G, 0, sizeof(G));
    G.n_query = nq;
    std::vector<int32_t> query((size_t)m), key((size_t)m);
    std::vector<int64_t> vals((size_t)m * (size_t)n_out);
    if (!rd(f, G.q, (size_t)nq * sizeof(sha_group_q)) || !rd(f, query.data(), query.size() * 4) ||
        !rd(f, key.data(), key.size() * 4) || !rd(f, vals.data(), vals.size() * 8))
        return 1;
    fclose(f);
    if (!shg_valid(&G, n_out)) return 1;
    struct full {
        int64_t q, k;
        uint64_t w[SH_MAX_GROUP];
        bool operator<(const full& o) const {
            if (q != o.q) return q < o.q;
            if (k != o.k) return k < o.k;
            for (int i = 0; i < SH_MAX_GROUP; i++)
                if (w[i] != o.w[i]) return w[i] < o.w[i];
            return false;
        }
    };
    std::vector<full> fk((size_t)m);
    for (int64_t r = 0; r < m; r++) {
        full& F = fk[(size_t)r];
        F.q = query[(size_t)r];
        F.k = key[(size_t)r];
        const sha_group_q* g = (F.q >= 0 && F.q < nq) ? &G.q[F.q] : nullptr;
        for (int i = 0; i < SH_MAX_GROUP; i++)
            F.w[i] = (g && i < g->n) ? shg_word(vals[(size_t)(r * n_out + g->col[i])], g->type[i]) : 0ull;
    }
    std::vector<int64_t> idx((size_t)m);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return fk[(size_t)a] < fk[(size_t)b]; });
    printf("order");
    for (int64_t p = 0; p < m; p++) printf(" %lld", (long long)idx[(size_t)p]);
    printf("\nseg");
    int64_t id = -1;
    for (int64_t p = 0; p < m; p++) {
        if (p == 0 || fk[(size_t)idx[(size_t)(p - 1)]] < fk[(size_t)idx[(size_t)p]]) id++;
        printf(" %lld", (long long)id);
    }
    printf("\n");
    return 0;
}
