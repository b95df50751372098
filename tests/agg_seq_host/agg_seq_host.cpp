// TEST INFRASTRUCTURE: the carried, sequential aggregate pass on the CPU. The
// arithmetic, the table key, the hash and the probe are the product's
// (siddhi_amd/csrc/sh_agg_seq.h, what k_shc_walk runs per segment); this file
// adds what the device does around them -- the stable order by (query, key), the
// segment heads, the insert and the table's growth -- in plain C++.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../siddhi_amd/csrc/sh_agg_seq.h"

namespace {
struct Host {
    sha_desc D;
    std::vector<uint64_t> keys;
    std::vector<int64_t> state;
    int64_t entries = 0;
    shq_table table() {
        shq_table T;
        memset(&T, 0, sizeof(T));
        T.keys = keys.data();
        T.state = state.data();
        T.cap = (int64_t)keys.size();
        T.n_cols = D.n_cols;
        return T;
    }
};

// insert or overwrite (the device claims the slot with a compare-and-swap)
void put(Host* H, std::vector<uint64_t>& keys, std::vector<int64_t>& state, uint64_t key, const int64_t* fin,
         int64_t* entries) {
    const int w = H->D.n_cols * 2;
    const uint64_t mask = (uint64_t)keys.size() - 1ull;
    uint64_t s = shq_hash(key) & mask;
    while (keys[s] != SHQ_EMPTY && keys[s] != key) s = (s + 1ull) & mask;
    if (keys[s] == SHQ_EMPTY) {
        keys[s] = key;
        (*entries)++;
    }
    for (int k = 0; k < w; k++) state[s * w + k] = fin[k];
}

void reserve(Host* H, int64_t add) {
    const int64_t need = (H->entries + add) * 2;
    if (!H->keys.empty() && need <= (int64_t)H->keys.size()) return;
    int64_t cap = std::max<int64_t>(1024, (int64_t)H->keys.size() * 2);
    while (cap < need) cap *= 2;
    const int w = H->D.n_cols * 2;
    std::vector<uint64_t> nk((size_t)cap, SHQ_EMPTY);
    std::vector<int64_t> ns((size_t)cap * w, 0);
    int64_t e = 0;
    for (size_t i = 0; i < H->keys.size(); i++)
        if (H->keys[i] != SHQ_EMPTY) put(H, nk, ns, H->keys[i], &H->state[i * w], &e);
    H->keys.swap(nk);
    H->state.swap(ns);
}
}  // namespace

extern "C" {
void* agq_create(int n_cols, const int32_t* col, const int32_t* kind, const int32_t* arg_type) {
    if (n_cols < 1 || n_cols > SHA_MAX_COLS) return nullptr;
    Host* H = new Host();
    memset(&H->D, 0, sizeof(H->D));
    H->D.n_cols = n_cols;
    for (int k = 0; k < n_cols; k++) {
        H->D.c[k].col = col[k];
        H->D.c[k].kind = kind[k];
        H->D.c[k].arg_type = arg_type[k];
    }
    return H;
}

// one step: vals [m x n_out] rows in output order with the aggregators' arguments
// in the aggregate columns become the running values; carry = 0 runs it from an
// empty table and keeps nothing
int agq_step(void* hv, int64_t* vals, int n_out, int64_t m, const int32_t* query, const int32_t* key, int carry) {
    Host* H = (Host*)hv;
    if (!H || m < 0 || n_out < 1) return -1;
    if (m == 0) return 0;
    const int nc = H->D.n_cols;
    if (carry) reserve(H, m);
    std::vector<uint64_t> seg((size_t)m);
    std::vector<uint32_t> idx((size_t)m);
    for (int64_t r = 0; r < m; r++) {
        seg[r] = shq_key(query ? query[r] : 0, key ? key[r] : 0);
        idx[r] = (uint32_t)r;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return seg[a] < seg[b]; });
    std::vector<int64_t> sc((size_t)nc * m), fin((size_t)nc * 2);
    for (int64_t p = 0; p < m; p++)
        for (int k = 0; k < nc; k++) sc[(size_t)k * m + p] = vals[(int64_t)idx[p] * n_out + H->D.c[k].col];
    shq_table none;
    memset(&none, 0, sizeof(none));
    for (int64_t p = 0; p < m;) {
        const uint64_t sg = seg[idx[p]];
        int64_t e = p + 1;
        while (e < m && seg[idx[e]] == sg) e++;
        const shq_table T = carry ? H->table() : none;
        const int64_t slot = shq_find(T, sg);
        for (int k = 0; k < nc; k++) shq_walk(sc.data() + (size_t)k * m, p, e, H->D.c[k], T, slot, k, &fin[k * 2]);
        if (carry) put(H, H->keys, H->state, sg, fin.data(), &H->entries);
        p = e;
    }
    for (int64_t p = 0; p < m; p++)
        for (int k = 0; k < nc; k++) vals[(int64_t)idx[p] * n_out + H->D.c[k].col] = sc[(size_t)k * m + p];
    return 0;
}

int64_t agq_entries(void* hv) { return hv ? ((Host*)hv)->entries : 0; }
int64_t agq_capacity(void* hv) { return hv ? (int64_t)((Host*)hv)->keys.size() : 0; }
void agq_destroy(void* hv) { delete (Host*)hv; }
}
