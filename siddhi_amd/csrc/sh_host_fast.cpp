// sh_host_fast.cpp -- drivers of the fast batch engines behind sh_run_device:
// the rule engine (sh_rules.hip; also its streaming step behind sh_push_batch,
// rules_stage / rules_step), the tile-local bucketed window engine and the
// sequence bucket-carry engine (sh_bucket.hip + shb_match), the aggregate post-pass
// (sh_agg.hip), and the key-segment helpers they share.
#include "sh_host_int.h"

int bits_for(uint64_t v) {
    int b = 0;
    while (b < 64 && (v >> b)) b++;
    return b;
}

shd_segment_ws seg_ws(sh_handle* h, int64_t n) {
    shd_segment_ws ws;
    ws.keys_a = h->w_keys_a.as<uint32_t>();
    ws.keys_b = h->w_keys_b.as<uint32_t>();
    ws.idx_a = h->w_idx_a.as<uint32_t>();
    ws.idx_b = h->w_idx_b.as<uint32_t>();
    ws.hist = h->w_hist.as<uint32_t>();
    ws.scan_tmp = h->w_scan.as<uint32_t>();
    ws.seg_off = h->w_seg.as<uint32_t>();
    ws.cap = n;
    return ws;
}

// ts and every column of stream 0 moved into key-segment order by the segment
// A 4-byte column that is the key array itself (the partition attribute, passed
// as the same device buffer) is not carried: its key-segment order is the
// sorted key array (*alias = that attribute, -1 if none). Null-key events
// (sorted to the sentinel bucket) are never read.
int carry_setup(sh_handle* h, const sh_device_run* run, shd_payload* carry, void** mid, int* alias,
                       bool used_only, bool with_ts) {
    const int64_t n = run->n;
    const int na = (int)h->stream_types[0].size();
    memset(carry, 0, sizeof(*carry));
    *alias = -1;
    int c = 0;
    if (with_ts) {
        if (h->v_sts.ensure_fresh(n * 8) || h->v_mid_ts.ensure_fresh(n * 8)) return SH_E_OOM;
        carry->src[c] = run->d_ts;
        carry->dst[c] = h->v_sts.p;
        carry->width[c] = 8;
        mid[c++] = h->v_mid_ts.p;
    }
    for (int a = 0; a < na; a++) {
        const int w = type_width(h->stream_types[0][a]);
        if (used_only && h->T && a < 32 && !((h->T->attr_used[0] >> a) & 1u)) continue;  // no expression reads it
        if (*alias < 0 && w == 4 && run->d_cols[a] == (const void*)run->d_keys && !getenv("SH_NO_KEY_ALIAS")) {
            *alias = a;
            continue;
        }
        if (h->v_scol[a].ensure_fresh(n * w) || h->v_mid[a].ensure_fresh(n * w)) return SH_E_OOM;
        carry->src[c] = run->d_cols[a];
        carry->dst[c] = h->v_scol[a].p;
        carry->width[c] = (uint8_t)w;
        mid[c++] = h->v_mid[a].p;
    }
    carry->n = c;
    return SH_OK;
}

// log2 of the arrival tile (0: untiled) for a partitioned window run: tiles of
// 2^19 events when the stream spans several and the directory stays small
// (SH_TILE_SHIFT overrides, for tests)
int tile_shift_for(int64_t n, int32_t nkeys) {
    int shift = 19;
    if (const char* e = getenv("SH_TILE_SHIFT")) shift = atoi(e);
    if (shift < 12 || shift > 24) return 0;
    const int64_t ntile = (n + ((int64_t)1 << shift) - 1) >> shift;
    if (ntile < 2 || ntile * ((int64_t)nkeys + 1) > ((int64_t)1 << 26)) return 0;
    return shift;
}

// ---- carried aggregates of a streaming rule set (sh_agg.hip, "carried, sequential pass")
static void agg_desc(const int32_t* agg_kind, const int32_t* arg_type, int n_out, sha_desc* D) {
    memset(D, 0, sizeof(*D));
    for (int o = 0; o < n_out && o < SHP_MAX_OUT && D->n_cols < SHA_MAX_COLS; o++)
        if (agg_kind[o] != SH_AGG_NONE) {
            D->c[D->n_cols].col = o;
            D->c[D->n_cols].kind = agg_kind[o];
            D->c[D->n_cols].arg_type = arg_type[o];
            D->n_cols++;
        }
}

int agg_carry_cols(const sh_handle* h) {
    sha_desc D;
    agg_desc(h->r_agg, h->r_argt, std::max(1, h->n_out), &D);
    return D.n_cols;
}

shq_table carry_table(const CarryTab& C) {
    shq_table T;
    memset(&T, 0, sizeof(T));
    T.keys = C.keys.as<uint64_t>();
    T.state = C.state.as<int64_t>();
    T.cap = C.cap;
    T.n_cols = C.ncols;
    return T;
}

// room for `add` more entries at no more than half full: the table is rebuilt at
// (at least) double capacity, every entry kept -- the one place a step costs O(table)
int carry_reserve(sh_handle* h, CarryTab& C, int64_t add, int n_cols) {
    hipStream_t st = h->stream;
    if (C.ctl.ensure_fresh(64)) return SH_E_OOM;
    const int64_t need = (C.entries + add) * 2;
    if (C.cap > 0 && need <= C.cap && C.ncols == n_cols) return SH_OK;
    int64_t cap = std::max<int64_t>(1024, C.cap * 2);
    while (cap < need) cap *= 2;
    DevBuf nk, nst;
    if (nk.ensure_fresh((size_t)cap * 8) || nst.ensure_fresh((size_t)cap * n_cols * 16)) {
        nk.release();
        nst.release();
        return SH_E_OOM;
    }
    hipMemsetAsync(nk.p, 0xFF, (size_t)cap * 8, st);  // SHQ_EMPTY
    hipMemsetAsync(C.ctl.p, 0, 16, st);
    int rc = 0;
    if (C.cap > 0 && C.entries > 0) {
        shq_table T;
        memset(&T, 0, sizeof(T));
        T.keys = nk.as<uint64_t>();
        T.state = nst.as<int64_t>();
        T.cap = cap;
        T.n_cols = n_cols;
        rc = shc_put(&T, C.keys.as<uint64_t>(), C.state.as<int64_t>(), C.cap, C.ctl.as<unsigned long long>(),
                     C.ctl.as<int32_t>() + 2, st);
    }
    uint64_t ctl[2] = {0, 0};
    hipMemcpyAsync(ctl, C.ctl.p, 16, hipMemcpyDeviceToHost, st);
    if (rc || hipStreamSynchronize(st) != hipSuccess || (ctl[1] & 1) || (int64_t)ctl[0] != C.entries) {
        nk.release();
        nst.release();
        return SH_E_HIP;
    }
    C.keys.release();
    C.state.release();
    C.keys = nk;
    C.state = nst;
    C.cap = cap;
    C.ncols = n_cols;
    return SH_OK;
}

// the table emptied and filled with n entries (restore; n = 0: a fresh handle's)
int carry_load(sh_handle* h, CarryTab& C, int nc, const uint64_t* keys, const int64_t* state, int64_t n) {
    hipStream_t st = h->stream;
    C.entries = 0;
    if (C.cap > 0) hipMemsetAsync(C.keys.p, 0xFF, (size_t)C.cap * 8, st);
    if (C.ctl.p) hipMemsetAsync(C.ctl.p, 0, 16, st);
    if (n <= 0) return hipStreamSynchronize(st) == hipSuccess ? SH_OK : SH_E_HIP;
    if (nc < 1) return SH_E_INVALID_ARG;
    if (carry_reserve(h, C, n, nc)) return SH_E_OOM;
    DevBuf dk, ds;
    int rc = SH_OK;
    uint64_t ctl[2] = {0, 0};
    if (dk.ensure_fresh((size_t)n * 8) || ds.ensure_fresh((size_t)n * nc * 16)) {
        rc = SH_E_OOM;
    } else {
        hipMemcpyAsync(dk.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(ds.p, state, (size_t)n * nc * 16, hipMemcpyHostToDevice, st);
        hipMemsetAsync(C.ctl.p, 0, 16, st);
        const shq_table T = carry_table(C);
        if (shc_put(&T, dk.as<uint64_t>(), ds.as<int64_t>(), n, C.ctl.as<unsigned long long>(),
                    C.ctl.as<int32_t>() + 2, st))
            rc = SH_E_HIP;
        hipMemcpyAsync(ctl, C.ctl.p, 16, hipMemcpyDeviceToHost, st);
        if (hipStreamSynchronize(st) != hipSuccess || (ctl[1] & 1)) rc = SH_E_HIP;
    }
    dk.release();
    ds.release();
    if (rc) return rc;
    if ((int64_t)ctl[0] != n) return SH_E_INVALID_ARG;  // (a key twice)
    C.entries = n;
    return SH_OK;
}

// the live entries sorted by table key, each with its per-column state
int carry_dump(const CarryTab& C, std::vector<uint64_t>& keys, std::vector<int64_t>& state) {
    keys.clear();
    state.clear();
    if (C.cap <= 0 || C.entries <= 0) return SH_OK;
    const size_t cap = (size_t)C.cap, w = (size_t)C.ncols * 2;
    std::vector<uint64_t> k(cap);
    std::vector<int64_t> s(cap * w);
    if (hipMemcpy(k.data(), C.keys.p, cap * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(s.data(), C.state.p, cap * w * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return SH_E_HIP;
    std::vector<size_t> live;
    for (size_t i = 0; i < cap; i++)
        if (k[i] != SHQ_EMPTY) live.push_back(i);
    std::sort(live.begin(), live.end(), [&](size_t a, size_t b) { return k[a] < k[b]; });
    for (size_t i : live) {
        keys.push_back(k[i]);
        state.insert(state.end(), s.begin() + i * w, s.begin() + (i + 1) * w);
    }
    return (int64_t)keys.size() == C.entries ? SH_OK : SH_E_HIP;
}

// sh_run_device on a rule set beyond the general engine's table whose additions
// would round in parallel: the sequential pass over the placed rows (left as
// placed by sha_running), every segment from zero -- a call's state is its own
static int agg_seq_bulk(sh_handle* h, sh_device_run* run, int32_t nkeys) {
    const int64_t m = run->out_count;
    const int no = std::max(1, h->n_out);
    sha_desc D;
    agg_desc(h->r_agg, h->r_argt, no, &D);
    if (m >= ((int64_t)1 << 31)) return fail(h, SH_E_UNSUPPORTED, "rule engine: 2^31 or more rows");
    if (h->a_scratch.ensure_fresh((size_t)shc_scratch_bytes(m, D.n_cols))) return fail(h, SH_E_OOM, "aggregate scratch");
    hipEventRecord(h->ev[4], h->stream);
    if (shc_running(run->d_out_seq, run->d_out_values, no, m, run->d_out_query, (int32_t)h->r_rules.size(), nullptr,
                    h->partitioned ? run->d_keys : nullptr, h->partitioned ? nkeys : 1, 0, &D, nullptr,
                    h->a_scratch.p, h->stream, nullptr, nullptr))
        return fail(h, SH_E_HIP, "sequential aggregate pass failed");
    hipEventRecord(h->ev[5], h->stream);
    if (hipEventSynchronize(h->ev[5]) != hipSuccess) return fail(h, SH_E_HIP, "device error in the aggregate pass");
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->ev[4], h->ev[5]);
    h->times.emit_ms += ms;
    h->times.total_ms += ms;
    h->agg_last = 6;
    return SH_OK;
}

// batch-compiled rule sets (sh_rules.hip) over HBM-resident columns

// the records' output order -- (run, query, consuming event), stable over the
// records' (opening event, rule) order; by_p: the records are in any order, so
// the first sort stage restores that order -- and the placed rows
static int rules_order_place(sh_handle* h, sh_device_run* run, int64_t m, const uint32_t* rec_p, const uint32_t* rec_q,
                             const uint32_t* rec_r, const uint32_t* perm, const int64_t* sts, const shd_cols* dC,
                             const uint32_t* sts32, int64_t tlo, bool sorted, bool by_p) {
    hipStream_t st = h->stream;
    const int64_t n = run->n;
    const shr_table* dT = h->rd_tab.as<shr_table>();
    const int64_t mt = (m + 4095) / 4096;
    const size_t sw = std::max(shd_scan_tmp_words(256 * mt), (size_t)16);
    if (h->r_keys.ensure_fresh((size_t)m * 12) || h->r_g.ensure_fresh((size_t)m * 8) ||
        h->r_sk.ensure_fresh((size_t)m * 8) || h->r_sv.ensure_fresh((size_t)m * 8) ||
        h->r_hist.ensure_fresh((size_t)256 * mt * 4 + 64) || h->r_scan.ensure_fresh(sw * 4 + 64))
        return fail(h, SH_E_OOM, "match records");
    // PartitionStreamReceiver runs inside each send() call
    const int64_t batch = run->batch_events > 0 ? run->batch_events : 0;
    const uint32_t* flags = nullptr;
    const uint32_t* rid = nullptr;
    const uint32_t* rfirst = nullptr;
    // the runs of the consuming events only, walked back from each record's event
    // (SH_RULES_RUNSCAN=1: flags, scan and first index over every event)
    const bool walk_runs = sorted && !getenv("SH_RULES_RUNSCAN");
    // order key (run, query, consuming event), least significant first; the
    // records are in (opening event, rule) order, which the stable sort keeps
    // among equal keys (creation order of the partials a consumer takes)
    const int64_t runlen = batch > 0 ? std::min(batch, n) : n;
    const int qbits = bits_for((uint64_t)(runlen - 1));
    const int rbits = bits_for((uint64_t)(h->r_rules.size() - 1));
    const int nbits = bits_for((uint64_t)(n - 1));
    const bool packed = qbits + rbits <= 32;
    uint32_t* k0 = h->r_keys.as<uint32_t>();
    uint32_t* k1 = k0 + m;
    uint32_t* k2 = k1 + m;
    bool scan_runs = sorted && !walk_runs;
    if (walk_runs) {
        int32_t* long_run = h->v_flag.as<int32_t>() + 1;
        int32_t lr = 0;
        hipMemsetAsync(long_run, 0, 4, st);
        if (shr_keys(rec_q, rec_r, m, perm, nullptr, nullptr, nullptr, batch, qbits, packed ? 1 : 0, k0, k1, k2,
                     st, run->d_keys, run->d_run, long_run))
            return fail(h, SH_E_HIP, "rule key launch failed");
        hipMemcpyAsync(&lr, long_run, 4, hipMemcpyDeviceToHost, st);
        if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in the rule keys");
        scan_runs = lr != 0;
    }
    if (scan_runs) {
        if (h->r_run.ensure_fresh((size_t)n * 12)) return fail(h, SH_E_OOM, "run ids");
        uint32_t* f = h->r_run.as<uint32_t>();
        if (shr_run_ids(run->d_keys, run->d_run, n, batch, f, f + n, f + 2 * n, h->w_scan.as<uint32_t>(), st))
            return fail(h, SH_E_HIP, "run id launch failed");
        flags = f;
        rid = f + n;
        rfirst = f + 2 * n;
    }
    if ((scan_runs || !walk_runs) &&
        shr_keys(rec_q, rec_r, m, perm, flags, rid, rfirst, batch, qbits, packed ? 1 : 0, k0, k1, k2, st))
        return fail(h, SH_E_HIP, "rule key launch failed");
    const uint32_t* stage_key[4];
    int stage_bits[4];
    int ns = 0;
    // by_p (records in any order): no stage by opening event -- four radix passes --
    // but the last stage's runs of equal keys put in rec_p order afterwards
    // (shr_order_ties; profiles/r6_c5_ties_ab.txt: advance -0.11 ms)
    const bool ties = by_p;
    if (packed) {
        stage_key[ns] = k0;
        stage_bits[ns++] = qbits + rbits;
    } else {
        stage_key[ns] = k0;
        stage_bits[ns++] = qbits;
        stage_key[ns] = k1;
        stage_bits[ns++] = rbits;
    }
    stage_key[ns] = packed ? k1 : k2;
    stage_bits[ns++] = nbits;
    const uint32_t* order = nullptr;
    uint32_t* gk = h->r_g.as<uint32_t>();
    uint32_t* gv = gk + m;
    uint32_t* kb[2] = {h->r_sk.as<uint32_t>(), h->r_sk.as<uint32_t>() + m};
    uint32_t* vb[2] = {h->r_sv.as<uint32_t>(), h->r_sv.as<uint32_t>() + m};
    for (int s = 0; s < ns; s++) {
        if (stage_bits[s] == 0) continue;
        const uint32_t* ko = nullptr;
        const uint32_t* vo = nullptr;
        if (shr_gather(stage_key[s], order, m, gk, gv, st) ||
            shd_sort_pairs(gk, gv, m, stage_bits[s], kb, vb, h->r_hist.as<uint32_t>(), h->r_scan.as<uint32_t>(),
                           st, &ko, &vo))
            return fail(h, SH_E_HIP, "rule sort launch failed");
        order = vo;
    }
    if (ties && !order) {  // (every stage empty: the identity order, in a buffer of ours)
        if (shr_gather(k0, nullptr, m, h->r_g.as<uint32_t>(), h->r_g.as<uint32_t>() + m, st))
            return fail(h, SH_E_HIP, "rule order launch failed");
        order = h->r_g.as<uint32_t>() + m;
    }
    if (ties &&
        shr_order_ties(const_cast<uint32_t*>(order), m, k0, k1, packed ? nullptr : k2, rec_p, st))
        return fail(h, SH_E_HIP, "rule order launch failed");
    hipEventRecord(h->ev[2], st);
    if (h->r_aggp) {
        if (!run->d_out_query) {
            if (h->a_q.ensure((size_t)m * 4)) return fail(h, SH_E_OOM, "aggregate query ids");
            run->d_out_query = h->a_q.as<int32_t>();
        }
        if (!run->d_out_seq) {
            if (h->a_seq.ensure((size_t)m * 8)) return fail(h, SH_E_OOM, "aggregate sequence numbers");
            run->d_out_seq = h->a_seq.as<uint64_t>();
        }
    }
    if (shr_place(dT, order, m, rec_p, rec_q, rec_r, perm, sts, dC, 0, std::max(1, h->n_out), run->d_out_seq,
                  run->d_out_query, h->step_ots, run->d_out_values, st, sts32, tlo, h->step_seqs))
        return fail(h, SH_E_HIP, "rule placement launch failed");
    // a step of an aggregating set: the partition key of every row's consuming event
    if (h->step_okey && shr_place_keys(order, m, rec_q, perm, run->d_keys, h->step_okey, st))
        return fail(h, SH_E_HIP, "rule placement launch failed");
    return SH_OK;
}

// the end of a rule run: kernel times, the aggregate post-pass
static int rules_finish(sh_handle* h, sh_device_run* run, int64_t m, int32_t nkeys) {
    hipStream_t st = h->stream;
    hipEventRecord(h->ev[3], st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in the rule engine");
    phase_times(h);
    h->times.advance_launches = 1;
    if (h->r_aggp && m > 0) {
        const int arc = agg_post(h, run, nkeys, run->d_out_query, (int)h->r_rules.size(), h->r_agg, h->r_argt,
                                 std::max(1, h->n_out));
        if (arc < 0) return arc;
        // not exact in parallel: the caller runs the general engine, which adds in
        // sequence; a set beyond its query table takes the sequential pass here
        if (arc == 1) return h->mode == 2 ? agg_seq_bulk(h, run, nkeys) : 1;
    }
    return SH_OK;
}

// partitioned rule sets whose start filters open few partials: no key segment
// (sh_rules.hip, "sparse partials"); 1 = not taken (decreasing timestamps, keys
// out of range, more partials than max(65536, n / 8) or than 64 per key): the
// caller runs the key-segment path.
// Phases: segment = the partials and their lists, advance = the consuming events
// and the records' order, emit = placement.
static int run_rules_sparse(sh_handle* h, sh_device_run* run, int32_t nkeys) {
    h->rs_last = 0;
    if (const char* e = getenv("SH_RULES_SPARSE"))
        if (e[0] == '0') return 1;
    hipStream_t st = h->stream;
    const int64_t n = run->n;
    if (n <= 1 || n >= (int64_t)0xFFFFFFFFll || !run->d_keys) return 1;
    if (h->r_rules.size() >= ((size_t)1 << 20)) return 1;  // (k_sparse_open's pairs hold 20-bit rule ids)
    const int64_t cap = std::max<int64_t>(65536, n / 8);
    const size_t nk1 = (size_t)nkeys + 1;
    if (h->rs_pr.ensure_fresh((size_t)cap * 16) || h->rs_key.ensure_fresh(nk1 * 12) ||
        h->rs_list.ensure_fresh((size_t)cap * 20) || h->rs_ctl.ensure_fresh(64) || ensure_ws(h, (int64_t)nk1))
        return fail(h, SH_E_OOM, "rule workspace");
    uint32_t* pr = h->rs_pr.as<uint32_t>();
    uint32_t* key_cnt = h->rs_key.as<uint32_t>();
    uint32_t* key_off = key_cnt + nk1;
    uint32_t* key_fill = key_off + nk1;
    unsigned long long* ctl = h->rs_ctl.as<unsigned long long>();  // [0] partials, [1] records, [2] flag
    shd_cols sc;
    memset(&sc, 0, sizeof(sc));
    const int na = (int)h->stream_types[0].size();
    for (int a = 0; a < na; a++) sc.col[0][a] = run->d_cols[a];
    hipEventRecord(h->ev[0], st);
    hipMemcpyAsync(h->d_cols_desc.p, &sc, sizeof(sc), hipMemcpyHostToDevice, st);
    const shd_cols* dC = h->d_cols_desc.as<shd_cols>();
    const shr_table* dT = h->rd_tab.as<shr_table>();
    hipMemsetAsync(key_cnt, 0, nk1 * 4, st);
    hipMemsetAsync(key_fill, 0, nk1 * 4, st);
    hipMemsetAsync(ctl, 0, 24, st);
    // the attributes the rules' terms read most on the opening event's row (f1) and on
    // the consumer's row (f2): loaded once per event by the sparse kernels
    int32_t pre_open[2] = {-1, -1}, pre_take[2] = {-1, -1};
    {
        int cnt0[32] = {0}, cnt1[32] = {0};
        for (const shr_rule& R : h->r_rules) {
            for (int t = 0; t < R.nt[0]; t++) {
                const shp_term& T = R.t[0][t];
                if (T.lslot == 0 && T.lattr >= 0 && T.lattr < 32) cnt0[T.lattr]++;
                if (T.rkind != 1 && T.rslot == 0 && T.rattr >= 0 && T.rattr < 32) cnt0[T.rattr]++;
            }
            for (int t = 0; t < R.nt[1]; t++) {
                const shp_term& T = R.t[1][t];
                if (T.lslot == 1 && T.lattr >= 0 && T.lattr < 32) cnt1[T.lattr]++;
                if (T.rkind != 1 && T.rslot == 1 && T.rattr >= 0 && T.rattr < 32) cnt1[T.rattr]++;
            }
        }
        auto top2 = [](const int* c, int32_t* out) {
            for (int k = 0; k < 2; k++) {
                int best = -1;
                for (int a = 0; a < 32; a++)
                    if (c[a] > 0 && a != out[0] && (best < 0 || c[a] > c[best])) best = a;
                out[k] = best;
            }
        };
        top2(cnt0, pre_open);
        top2(cnt1, pre_take);
    }
    if (shr_sparse_open(dT, run->d_ts, run->d_keys, n, nkeys, dC, h->r_img.bytes ? h->rd_img.as<uint8_t>() : nullptr,
                        &h->r_img, pr, pr + cap, pr + 2 * cap, key_cnt, ctl, cap, (int32_t*)(ctl + 2), pre_open,
                        st))
        return fail(h, SH_E_HIP, "sparse partial launch failed");
    unsigned long long rd[5] = {0, 0, 0, 0, 0};
    hipMemcpyAsync(rd, ctl, 24, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(rd + 3, run->d_ts, 8, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(rd + 4, run->d_ts + (n - 1), 8, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in the sparse partials");
    const int64_t np = (int64_t)rd[0];
    // a key's events each test all of its key's partials: dense partials per key take
    // the key-segment path (whose walk stops at each partial's window)
    if (rd[2] || np > cap || np > (int64_t)64 * nkeys) return 1;
    if (shd_exclusive_scan(key_cnt, key_off, (int64_t)nk1, h->w_scan.as<uint32_t>(), st))
        return fail(h, SH_E_HIP, "scan");
    hipEventRecord(h->ev[1], st);
    uint32_t* l_p = h->rs_list.as<uint32_t>();
    uint32_t* l_r = l_p + cap;
    uint32_t* l_q = l_r + cap;
    int64_t* l_te = (int64_t*)(l_q + cap);
    const int64_t rcap = std::max<int64_t>(np, 1);
    if (h->r_rec.ensure_fresh((size_t)rcap * 12)) return fail(h, SH_E_OOM, "match records");
    // the live-partial bitmap (shr_live): the run's time span in <= SH_SPARSE_SLICES
    // (default 256) power-of-two slices, one bit per key and slice (SH_SPARSE_LIVE=0: off)
    shr_live LV;
    memset(&LV, 0, sizeof(LV));
    {
        static const bool live_off = getenv("SH_SPARSE_LIVE") && getenv("SH_SPARSE_LIVE")[0] == '0';
        static const int max_sl = getenv("SH_SPARSE_SLICES") ? std::max(1, atoi(getenv("SH_SPARSE_SLICES"))) : 256;
        const int64_t tmin = (int64_t)rd[3], span = (int64_t)rd[4] - tmin + 1;
        if (!live_off && span > 0) {
            int shift = 0;
            while (shift < 62 && ((span - 1) >> shift) + 1 > max_sl) shift++;
            LV.tmin = tmin;
            LV.shift = shift;
            LV.nslices = (int32_t)(((span - 1) >> shift) + 1);
            LV.wps = (nkeys + 31) / 32;
            const size_t bytes = (size_t)LV.nslices * LV.wps * 4;
            if (h->rs_live.ensure(bytes)) return fail(h, SH_E_OOM, "live bitmap");
            LV.bits = h->rs_live.as<uint32_t>();
            hipMemsetAsync(LV.bits, 0, bytes, st);
        }
    }
    uint32_t* rec_p = h->r_rec.as<uint32_t>();
    uint32_t* rec_q = rec_p + rcap;
    uint32_t* rec_r = rec_q + rcap;
    if (np > 0 &&
        shr_sparse_match(dT, run->d_ts, run->d_keys, n, dC, h->r_img.bytes ? h->rd_img.as<uint8_t>() : nullptr,
                         &h->r_img, pr, pr + cap, pr + 2 * cap, key_fill, ctl, np, key_off,
                         l_p, l_r, l_te, l_q, rec_p, rec_q, rec_r, ctl + 1, rcap, nkeys, &LV, pre_take, st))
        return fail(h, SH_E_HIP, "sparse match launch failed");
    hipMemcpyAsync(rd, ctl, 16, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in the sparse match");
    const int64_t m = (int64_t)rd[1];
    h->rs_last = 1;
    run->out_count = m;
    if (m > run->out_capacity) return fail(h, SH_E_MORE, "output capacity too small");
    if (m > 0) {
        // the records' arrays hold rcap entries each: compact them for the order stages
        if (m < rcap) {
            hipMemcpyAsync(rec_p + m, rec_q, (size_t)m * 4, hipMemcpyDeviceToDevice, st);
            hipMemcpyAsync(rec_p + 2 * m, rec_r, (size_t)m * 4, hipMemcpyDeviceToDevice, st);
        }
        int prc = rules_order_place(h, run, m, rec_p, rec_p + m, rec_p + 2 * m, nullptr, run->d_ts, dC, nullptr, 0,
                                    true, true);
        if (prc) return prc;
    } else {
        hipEventRecord(h->ev[2], st);
    }
    return rules_finish(h, run, m, nkeys);
}

int run_rules(sh_handle* h, sh_device_run* run) {
    hipStream_t st = h->stream;
    const int64_t n = run->n;
    const int na = (int)h->stream_types[0].size();
    if (na > 7) return fail(h, SH_E_UNSUPPORTED, "rule engine: at most 7 attributes per stream");
    const bool sorted = h->r_partitioned;
    const int32_t nkeys = sorted ? std::max(1, run->n_keys) : 1;
    if (ensure_ws(h, n) || h->v_flag.ensure_fresh(64)) return fail(h, SH_E_OOM, "workspace");
    h->times = sh_kernel_times{};
    if (sorted) {
        const int src = run_rules_sparse(h, run, nkeys);
        if (src != 1) return src;
    }
    shd_batch B;
    memset(&B, 0, sizeof(B));
    B.ts = run->d_ts;
    B.keys = sorted ? run->d_keys : nullptr;
    B.n = n;
    shd_payload carry;
    void* mid[8] = {nullptr};
    int alias = -1;
    hipEventRecord(h->ev[0], st);
    // SH_RULES_TS32=1: timestamps travel through the segment as 32-bit offsets from
    // the run's first time when its range fits (4 bytes fewer per event and pass).
    // Off by default: on C5 the three passes gained 0.35 ms, the range and
    // conversion passes cost 0.66 ms (profiles/r3_c5_ts32_ab.txt)
    int64_t tlo = 0, thi = 0;
    bool ts32 = false;
    if (sorted && getenv("SH_RULES_TS32") && getenv("SH_RULES_TS32")[0] == '1') {
        if (h->r_tsr.ensure_fresh(64)) return fail(h, SH_E_OOM, "rule workspace");
        if (shr_ts_range(run->d_ts, n, &tlo, &thi, h->r_tsr.p, st)) return fail(h, SH_E_HIP, "timestamp range");
        ts32 = thi >= tlo && (uint64_t)(thi - tlo) <= 0xFFFFFFFFull;
    }
    if (sorted && carry_setup(h, run, &carry, mid, &alias, false, !ts32)) return fail(h, SH_E_OOM, "rule workspace");
    if (ts32) {
        if (h->v_ts32.ensure_fresh((size_t)n * 4) || h->v_sts32.ensure_fresh((size_t)n * 4) ||
            h->v_mid_ts32.ensure_fresh((size_t)n * 4))
            return fail(h, SH_E_OOM, "rule workspace");
        if (shr_ts_to32(run->d_ts, n, tlo, h->v_ts32.as<uint32_t>(), st)) return fail(h, SH_E_HIP, "timestamps");
        carry.src[carry.n] = h->v_ts32.p;
        carry.dst[carry.n] = h->v_sts32.p;
        carry.width[carry.n] = 4;
        mid[carry.n] = h->v_mid_ts32.p;
        carry.n++;
    }
    const uint32_t* sts32 = ts32 ? h->v_sts32.as<uint32_t>() : nullptr;
    shd_segment_ws ws = seg_ws(h, n);
    const uint32_t* perm = nullptr;
    const uint32_t* skeys = nullptr;
    if (shd_segment_payload(&B, nkeys, &ws, st, &perm, &skeys, sorted ? &carry : nullptr, mid, 0, 0))
        return fail(h, SH_E_HIP, "segment launch failed");
    hipEventRecord(h->ev[1], st);
    const int64_t* sts = ts32 ? nullptr : (sorted ? h->v_sts.as<int64_t>() : run->d_ts);
    shd_cols sc;
    memset(&sc, 0, sizeof(sc));
    for (int a = 0; a < na; a++) sc.col[0][a] = sorted ? (const void*)h->v_scol[a].p : run->d_cols[a];
    if (alias >= 0) sc.col[0][alias] = skeys;
    hipMemcpyAsync(h->d_cols_desc.p, &sc, sizeof(sc), hipMemcpyHostToDevice, st);
    const shd_cols* dC = h->d_cols_desc.as<shd_cols>();
    const shr_table* dT = h->rd_tab.as<shr_table>();
    const uint32_t sentinel = sorted ? (uint32_t)nkeys : 0xFFFFFFFFu;
    uint32_t* cnt = h->w_cnt.as<uint32_t>();
    uint32_t* off = h->w_off.as<uint32_t>();
    hipMemsetAsync(h->v_flag.p, 0, 4, st);
    if (shr_count(dT, sts, skeys, n, sentinel, dC, cnt, h->v_flag.as<int32_t>(), st,
                  h->r_img.bytes ? h->rd_img.as<uint8_t>() : nullptr, &h->r_img, sts32, tlo) ||
        shd_exclusive_scan(cnt, off, n, h->w_scan.as<uint32_t>(), st))
        return fail(h, SH_E_HIP, "rule scan launch failed");
    uint32_t lo = 0, lc = 0;
    int32_t flag = 0;
    hipMemcpyAsync(&lo, off + (n - 1), 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&lc, cnt + (n - 1), 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&flag, h->v_flag.p, 4, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in the rule scan");
    if (flag) return fail(h, SH_E_UNSUPPORTED, "rule engine: timestamps decrease inside a key");
    const int64_t m = (int64_t)lo + lc;
    run->out_count = m;
    if (m > run->out_capacity) return fail(h, SH_E_MORE, "output capacity too small");
    if (m > 0) {
        if (h->r_rec.ensure_fresh((size_t)m * 12)) return fail(h, SH_E_OOM, "match records");
        uint32_t* rec_p = h->r_rec.as<uint32_t>();
        uint32_t* rec_q = rec_p + m;
        uint32_t* rec_r = rec_q + m;
        if (shr_write(dT, sts, skeys, n, sentinel, dC, cnt, off, rec_p, rec_q, rec_r, st,
                      h->r_img.bytes ? h->rd_img.as<uint8_t>() : nullptr, &h->r_img, sts32, tlo))
            return fail(h, SH_E_HIP, "rule write launch failed");
        int prc = rules_order_place(h, run, m, rec_p, rec_q, rec_r, perm, sts, dC, sts32, tlo, sorted, false);
        if (prc) return prc;
    } else {
        hipEventRecord(h->ev[2], st);
    }
    return rules_finish(h, run, m, nkeys);
}

// ---- streaming rule sets (mode 2): sh_push_batch stages, flush runs one step
//
// One send(Event[]) call of a rule set beyond the general engine's table. The keyed
// events are appended to the host staging with their own sequence numbers (a
// null-key event is dropped but takes a number) and their PartitionStreamReceiver
// run: the consecutive same-key events of the call, or the whole call when
// unpartitioned. A dropped event ends the run around it, as it does for the general
// engine's streaming path (sh_nfa.hip joins(): a run's events are adjacent in the
// call) and for the oracle, so a rule set orders its rows the same on either side of
// the 16-query table. (The bulk path's k_run_flags skips such an event inside a run.)
int rules_stage(sh_handle* h, const sh_batch* b) {
    const auto& types = h->stream_types[0];
    const int na = (int)types.size();
    if (na > 7) return fail(h, SH_E_UNSUPPORTED, "rule engine: at most 7 attributes per stream");
    if (h->rq_ts.empty() && !h->rq_nullbit) h->rq_call0 = h->rq_call;
    if (b->nulls)
        for (int a = 0; a < na && !h->rq_nullbit; a++)
            if (b->nulls[a])
                for (int64_t i = 0; i < b->n; i++)
                    if (b->nulls[a][i]) {
                        h->rq_nullbit = true;
                        break;
                    }
    bool any = false, dropped = false;
    int32_t prev = -1;
    const size_t at = h->rq_ts.size();
    for (int64_t i = 0; i < b->n; i++) {
        const int32_t k = h->partitioned ? (b->keys ? b->keys[i] : -1) : 0;
        if (k < 0) {
            dropped = true;
            prev = -1;  // the next keyed event starts a run
            continue;
        }
        if (!any || (h->partitioned && k != prev)) h->rq_run_next++;
        any = true;
        prev = k;
        h->rq_ts.push_back(b->ts[i]);
        h->rq_key.push_back(k);
        h->rq_seq.push_back(h->seq_next + (uint64_t)i);
        h->rq_run.push_back(h->rq_run_next);
        if (k + 1 > h->max_key) h->max_key = k + 1;
    }
    for (int a = 0; a < na; a++) {
        const size_t w = (size_t)type_width(types[a]);
        const uint8_t* src = (const uint8_t*)b->cols[a];
        if (!dropped) {  // the whole column at once
            h->rq_col[a].insert(h->rq_col[a].end(), src, src + (size_t)b->n * w);
            continue;
        }
        for (size_t j = at; j < h->rq_ts.size(); j++) {
            const size_t i = (size_t)(h->rq_seq[j] - h->seq_next);
            h->rq_col[a].insert(h->rq_col[a].end(), src + i * w, src + (i + 1) * w);
        }
    }
    h->seq_next += (uint64_t)b->n;
    h->rq_call++;
    return SH_OK;
}

// the device row filter (sh_having.hip) over m ordered raw rows, launched on the
// handle's stream: the kept rows go to dst, their count to h->hv.kept
int having_filter(sh_handle* h, int64_t m, int n_out, const shw_rows& src, const shw_rows_out& dst) {
    RowStage& S = h->hv;
    if (S.ws.ensure_fresh((size_t)shv_filter_ws_words(m) * 4) || S.kept.ensure(64))
        return fail(h, SH_E_OOM, "having filter workspace");
    for (auto& e : S.ev)
        if (!e) hipEventCreate(&e);
    hipEventRecord(S.ev[0], h->stream);
    if (shv_filter(h->hv_d_progs.as<shv_prog>(), (int32_t)h->hv_progs.size(), m, n_out, &src, &dst, S.ws.as<uint32_t>(),
                   S.kept.as<unsigned long long>(), h->stream))
        return fail(h, SH_E_HIP, "having filter launch failed");
    hipEventRecord(S.ev[1], h->stream);
    return SH_OK;
}

int rate_limit(sh_handle* h, int64_t m, int n_out, const shw_rows& src, const int32_t* keys, int32_t n_keys,
               const shq_table* T, const shw_rows_out& dst, const uint64_t** put_keys, const int64_t** put_state) {
    RowStage& S = h->rl;
    if (S.ws.ensure_fresh((size_t)shl_limit_ws_words(m) * 4) || S.kept.ensure(64))
        return fail(h, SH_E_OOM, "event limiter workspace");
    for (auto& e : S.ev)
        if (!e) hipEventCreate(&e);
    hipEventRecord(S.ev[0], h->stream);
    if (shl_limit_rules(h->rl_rules.data(), h->rl_d_rules.as<shl_rule>(), (int32_t)h->rl_rules.size(), m, n_out, &src,
                        keys, n_keys, 0, T, &dst, S.ws.as<uint32_t>(), S.kept.as<unsigned long long>(), h->stream,
                        put_keys, put_state))
        return fail(h, SH_E_HIP, "event limiter launch failed");
    hipEventRecord(S.ev[1], h->stream);
    return SH_OK;
}

// the host output queue at `rows` rows (a step appends its rows, or takes them back)
static void out_queue_rows(sh_handle* h, size_t rows) {
    h->o_query.resize(rows);
    h->o_seq.resize(rows);
    h->o_ts.resize(rows);
    h->o_vals.resize(rows * h->n_out);
    h->o_nulls.resize(rows * h->n_out, 0);
}

// a step's staged calls are behind it: the staging emptied, and the counters where
// the next calls start (the step's end, or -- a refused step -- where they were before)
static void rules_unstage(sh_handle* h) {
    h->rq_ts.clear();
    h->rq_key.clear();
    h->rq_seq.clear();
    h->rq_run.clear();
    for (auto& c : h->rq_col) c.clear();
    h->rq_run_next = 0;
    h->seq_staged0 = h->seq_next;
    h->rq_call0 = h->rq_call;
}

// the staged calls are dropped: a refused step leaves the handle where it was
// before them (counters included), with the carried state untouched
static int rules_step_fail(sh_handle* h, int code, const char* msg) {
    h->seq_next = h->seq_staged0;
    h->rq_call = h->rq_call0;
    rules_unstage(h);
    h->rq_nullbit = false;
    h->step_seqs = nullptr;
    h->step_ots = nullptr;
    h->step_okey = nullptr;
    return fail(h, code, msg);
}

// the stage's own destination for `rows` rows in S's buffers: every column src has
static int stage_rows(RowStage& S, size_t rows, int n_out, const shw_rows& src, bool with_key, shw_rows_out* o) {
    if (S.vals.ensure_fresh(rows * n_out * 8) || (src.seq && S.seq.ensure_fresh(rows * 8)) ||
        (src.query && S.q.ensure_fresh(rows * 4)) || (src.ts && S.ts.ensure_fresh(rows * 8)) ||
        (with_key && S.key.ensure_fresh(rows * 4)))
        return SH_E_OOM;
    *o = shw_rows_out{src.seq ? S.seq.as<uint64_t>() : nullptr,
                      S.vals.as<int64_t>(),
                      src.query ? S.q.as<int32_t>() : nullptr,
                      src.ts ? S.ts.as<int64_t>() : nullptr,
                      nullptr,
                      with_key ? S.key.as<int32_t>() : nullptr};
    return SH_OK;
}

int row_post(sh_handle* h, RowPost& P) {
    auto refuse = [&](int code, const char* msg) { return P.step ? rules_step_fail(h, code, msg) : fail(h, code, msg); };
    shw_rows src = P.src;
    int64_t m = P.m;
    for (int pass = 0; pass < 2; pass++) {
        const bool rate = pass == 1;
        if (rate) P.after_having = m;
        if (!(rate ? h->rl_on : h->hv_on) || (rate && P.step && m == 0)) continue;
        RowStage& S = rate ? h->rl : h->hv;
        const bool last = rate || !h->rl_on;
        shw_rows_out dst;
        if (last && P.end)
            dst = *P.end;
        else if (stage_rows(last ? S : *P.mid, P.room ? P.room : (size_t)m, P.n_out, src, !last && src.key, &dst))
            return refuse(SH_E_OOM, !P.step ? "row filter buffers" : rate ? "event limiter buffers" : "having filter buffers");
        int rc;
        if (rate) {
            shq_table T;
            if (P.tab) T = carry_table(*P.tab);
            rc = rate_limit(h, m, P.n_out, src, P.d_keys, P.n_keys, P.tab ? &T : nullptr, dst,
                            P.tab ? &P.put_keys : nullptr, P.tab ? &P.put_state : nullptr);
        } else {
            rc = having_filter(h, m, P.n_out, src, dst);
        }
        if (rc) return P.step ? rules_step_fail(h, SH_E_HIP, h->err.c_str()) : rc;
        unsigned long long kept = 0;
        hipMemcpyAsync(&kept, S.kept.p, 8, hipMemcpyDeviceToHost, h->stream);
        if (hipStreamSynchronize(h->stream) != hipSuccess || (int64_t)kept > m)
            return refuse(SH_E_HIP, rate ? "device error in the event limiters" : "device error in the having filter");
        if (!P.step) {
            S.last = 1;
            S.rows_in = m;
            S.rows_kept = (int64_t)kept;
        }
        m = (int64_t)kept;
        src = shw_rows{dst.seq, dst.vals, dst.query, dst.ts, dst.nulls, dst.key};
    }
    P.after_rate = m;
    P.out = src;
    return SH_OK;
}

// One device step over everything staged: the key-segment scans run over the
// carried opening events followed by the staged events (shr_carry), the records
// are ordered and placed as in run_rules and appended to the host output queue,
// and the survivors become the next carried state in the other store. The sparse
// path is not taken: it keeps no survivors.
int rules_step(sh_handle* h) {
    if (h->rq_ts.empty() && !h->rq_nullbit) {
        h->seq_staged0 = h->seq_next;  // (calls of null-key events only)
        h->rq_call0 = h->rq_call;
        return SH_OK;
    }
    if (h->rq_nullbit)
        return rules_step_fail(h, SH_E_UNSUPPORTED, "rule engine: null attribute values are not supported");
    h->stream = h->own_stream;
    hipStream_t st = h->stream;
    const auto& types = h->stream_types[0];
    const int na = (int)types.size();
    const int64_t ns = (int64_t)h->rq_ts.size(), nc = h->rc_rows, n = nc + ns;
    if (n >= 0x7FFFFFFFll) return rules_step_fail(h, SH_E_UNSUPPORTED, "rule engine: carried plus staged rows >= 2^31");
    const bool sorted = h->r_partitioned;
    const int32_t nkeys = sorted ? std::max(1, h->max_key) : 1;
    sh_handle::RuleStore& A = h->rc[h->rc_cur];
    sh_handle::RuleStore& Bn = h->rc[1 - h->rc_cur];
    int oom = A.ts.ensure((size_t)n * 8) | A.key.ensure((size_t)n * 4) | A.seq.ensure((size_t)n * 8) |
              A.run.ensure((size_t)n * 4) | A.c_off.ensure(((size_t)nc + 1) * 4) | A.c_rule.ensure(4);
    for (int a = 0; a < na; a++) oom |= A.col[a].ensure((size_t)n * type_width(types[a]));
    if (nkeys > h->rc_nkeys) {
        const int32_t nk = std::max(nkeys, h->rc_nkeys * 2);
        oom |= h->rc_klast.ensure((size_t)nk * 8);
        if (!oom && shr_fill_i64(h->rc_klast.as<int64_t>() + h->rc_nkeys, nk - h->rc_nkeys, INT64_MIN, st)) oom = 1;
        if (!oom) h->rc_nkeys = nk;
    }
    const int64_t nb = shr_carry_blocks(n);
    // workspace: scnt [n + 1], soff [n + 1], lid [n], blk [nb + 1], blk_off [nb + 1]
    oom |= h->rc_ws.ensure_fresh(((size_t)3 * n + 2 * nb + 8) * 4);
    if (oom || ensure_ws(h, std::max(n + 1, nb + 1)) || h->v_flag.ensure_fresh(64))
        return rules_step_fail(h, SH_E_OOM, "rule step workspace");
    if (nc == 0) hipMemsetAsync(A.c_off.p, 0, 4, st);
    hipMemsetAsync(A.run.p, 0, (size_t)nc * 4, st);  // carried rows: run 0, never a consumer's
    hipMemcpyAsync(A.ts.as<int64_t>() + nc, h->rq_ts.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A.key.as<int32_t>() + nc, h->rq_key.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A.seq.as<uint64_t>() + nc, h->rq_seq.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(A.run.as<uint32_t>() + nc, h->rq_run.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st);
    const void* colp[8] = {nullptr};
    for (int a = 0; a < na; a++) {
        const size_t w = (size_t)type_width(types[a]);
        hipMemcpyAsync(A.col[a].as<uint8_t>() + (size_t)nc * w, h->rq_col[a].data(), (size_t)ns * w,
                       hipMemcpyHostToDevice, st);
        colp[a] = A.col[a].p;
    }
    h->times = sh_kernel_times{};
    sh_device_run R;
    memset(&R, 0, sizeof(R));
    R.n = n;
    R.d_ts = A.ts.as<int64_t>();
    R.d_keys = A.key.as<int32_t>();
    R.n_keys = nkeys;
    R.d_cols = colp;
    R.d_run = A.run.as<uint32_t>();
    shd_batch B;
    memset(&B, 0, sizeof(B));
    B.ts = R.d_ts;
    B.keys = sorted ? R.d_keys : nullptr;
    B.n = n;
    shd_payload carry;
    void* mid[8] = {nullptr};
    int alias = -1;
    hipEventRecord(h->ev[0], st);
    if (sorted && carry_setup(h, &R, &carry, mid, &alias, false, true))
        return rules_step_fail(h, SH_E_OOM, "rule step workspace");
    shd_segment_ws ws = seg_ws(h, n);
    const uint32_t* perm = nullptr;
    const uint32_t* skeys = nullptr;
    if (shd_segment_payload(&B, nkeys, &ws, st, &perm, &skeys, sorted ? &carry : nullptr, mid, 0, 0))
        return rules_step_fail(h, SH_E_HIP, "segment launch failed");
    hipEventRecord(h->ev[1], st);
    const int64_t* sts = sorted ? h->v_sts.as<int64_t>() : R.d_ts;
    shd_cols sc;
    memset(&sc, 0, sizeof(sc));
    for (int a = 0; a < na; a++) sc.col[0][a] = sorted ? (const void*)h->v_scol[a].p : colp[a];
    if (alias >= 0) sc.col[0][alias] = skeys;
    hipMemcpyAsync(h->d_cols_desc.p, &sc, sizeof(sc), hipMemcpyHostToDevice, st);
    const shd_cols* dC = h->d_cols_desc.as<shd_cols>();
    const shr_table* dT = h->rd_tab.as<shr_table>();
    const uint32_t sentinel = sorted ? (uint32_t)nkeys : 0xFFFFFFFFu;
    uint32_t* cnt = h->w_cnt.as<uint32_t>();
    uint32_t* off = h->w_off.as<uint32_t>();
    uint32_t* scnt = h->rc_ws.as<uint32_t>();
    uint32_t* soff = scnt + (n + 1);
    uint32_t* lid = soff + (n + 1);
    uint32_t* blk = lid + n;
    uint32_t* blk_off = blk + (nb + 1);
    shr_carry K;
    memset(&K, 0, sizeof(K));
    K.nc = (uint32_t)nc;
    K.perm = perm;
    K.c_off = A.c_off.as<uint32_t>();
    K.c_rule = A.c_rule.as<uint32_t>();
    K.klast = h->rc_klast.as<int64_t>();
    K.scnt = scnt;
    const uint8_t* img = h->r_img.bytes ? h->rd_img.as<uint8_t>() : nullptr;
    hipMemsetAsync(h->v_flag.p, 0, 8, st);
    hipMemsetAsync(cnt, 0, (size_t)n * 4, st);
    hipMemsetAsync(scnt, 0, ((size_t)n + 1) * 4, st);
    hipMemsetAsync(blk + nb, 0, 4, st);
    if (shr_count(dT, sts, skeys, n, sentinel, dC, cnt, h->v_flag.as<int32_t>(), st, img, &h->r_img, nullptr, 0, &K) ||
        shd_exclusive_scan(cnt, off, n, h->w_scan.as<uint32_t>(), st) ||
        shd_exclusive_scan(scnt, soff, n + 1, h->w_scan.as<uint32_t>(), st) || shr_carry_ids(scnt, n, lid, blk, st) ||
        shd_exclusive_scan(blk, blk_off, nb + 1, h->w_scan.as<uint32_t>(), st))
        return rules_step_fail(h, SH_E_HIP, "rule scan launch failed");
    uint32_t lo = 0, lc = 0, npairs = 0, nrows = 0;
    int32_t flag = 0;
    const uint64_t* ag_pk = nullptr;   // carried aggregates: the step's segment heads and
    const int64_t* ag_fin = nullptr;   // their final states (shc_running)
    RowPost post;                      // event limiters: the step's runs and their next
                                       // counters (shl_limit) come back in put_keys / put_state
    hipMemcpyAsync(&lo, off + (n - 1), 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&lc, cnt + (n - 1), 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&npairs, soff + n, 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&nrows, blk_off + nb, 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(&flag, h->v_flag.p, 4, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return rules_step_fail(h, SH_E_HIP, "device error in the rule scan");
    if (flag) return rules_step_fail(h, SH_E_UNSUPPORTED, "rule engine: timestamps decrease inside a key");
    const int64_t m = (int64_t)lo + lc;
    int64_t mk = m;   // the rows that reach the host queue (after `having` and the event limiters)
    int64_t ml = 0;   // ... that reached the limiters (after `having`)
    // the next carried state, beside the current one
    oom = Bn.ts.ensure_fresh(std::max<size_t>(nrows, 1) * 8) | Bn.key.ensure_fresh(std::max<size_t>(nrows, 1) * 4) |
          Bn.seq.ensure_fresh(std::max<size_t>(nrows, 1) * 8) | Bn.c_off.ensure_fresh(((size_t)nrows + 1) * 4) |
          Bn.c_rule.ensure_fresh(std::max<size_t>(npairs, 1) * 4);
    void* cdst[8] = {nullptr};
    int32_t cw[8] = {0};
    for (int a = 0; a < na; a++) {
        cw[a] = type_width(types[a]);
        oom |= Bn.col[a].ensure_fresh(std::max<size_t>(nrows, 1) * cw[a]);
        cdst[a] = Bn.col[a].p;
    }
    if (oom || h->r_rec.ensure_fresh((size_t)std::max<int64_t>(m, 1) * 12))
        return rules_step_fail(h, SH_E_OOM, "rule step state");
    K.soff = soff;
    K.s_rule = Bn.c_rule.as<uint32_t>();
    uint32_t* rec_p = h->r_rec.as<uint32_t>();
    uint32_t* rec_q = rec_p + m;
    uint32_t* rec_r = rec_q + m;
    if ((m > 0 || npairs > 0) &&
        shr_write(dT, sts, skeys, n, sentinel, dC, cnt, off, rec_p, rec_q, rec_r, st, img, &h->r_img, nullptr, 0, &K))
        return rules_step_fail(h, SH_E_HIP, "rule write launch failed");
    const int no = std::max(1, h->n_out);
    const bool rl_keyed = h->rl_on && sorted;  // the limiters' runs are per (query, partition key)
    if (m > 0) {
        if (h->w_oseq.ensure_fresh((size_t)m * 8) || h->rc_ots.ensure_fresh((size_t)m * 8) ||
            h->rc_oq.ensure_fresh((size_t)m * 4) || h->w_ovals.ensure_fresh((size_t)m * no * 8))
            return rules_step_fail(h, SH_E_OOM, "output buffers");
        R.d_out_seq = h->w_oseq.as<uint64_t>();
        R.d_out_query = h->rc_oq.as<int32_t>();
        R.d_out_values = h->w_ovals.as<int64_t>();
        R.out_capacity = m;
        sha_desc AD;
        if (h->r_aggp) {
            // carried aggregates: the trigger keys ride along with the placement, the
            // table has room for a new segment per row before anything reads it (a
            // rebuild keeps every entry, so a refusal further down loses nothing)
            agg_desc(h->r_agg, h->r_argt, no, &AD);
            if ((sorted && h->rc_okey.ensure_fresh((size_t)m * 4)) ||
                h->a_scratch.ensure_fresh((size_t)shc_scratch_bytes(m, AD.n_cols)) || carry_reserve(h, h->ag_tab, m, AD.n_cols))
                return rules_step_fail(h, SH_E_OOM, "carried aggregates");
            h->step_okey = sorted ? h->rc_okey.as<int32_t>() : nullptr;
        }
        if (h->rl_on) {
            // the limiters' counters: keyed and reserved as the aggregates' states are
            if ((sorted && h->rc_okey.ensure_fresh((size_t)m * 4)) || carry_reserve(h, h->rl_tab, m, 1))
                return rules_step_fail(h, SH_E_OOM, "carried limiter counters");
            h->step_okey = sorted ? h->rc_okey.as<int32_t>() : nullptr;
        }
        h->step_seqs = A.seq.as<uint64_t>();
        h->step_ots = h->rc_ots.as<int64_t>();
        // (runs from the staged events' run ids, for unpartitioned sets too)
        const int prc = rules_order_place(h, &R, m, rec_p, rec_q, rec_r, perm, sts, dC, nullptr, 0, true, false);
        h->step_seqs = nullptr;
        h->step_ots = nullptr;
        h->step_okey = nullptr;
        if (prc) return rules_step_fail(h, prc, h->err.c_str());
        // the running values, one addition at a time from each segment's carried state
        // (the table itself moves last, below)
        if (h->r_aggp) {
            const shq_table T = carry_table(h->ag_tab);
            if (shc_running(h->w_oseq.as<uint64_t>(), h->w_ovals.as<int64_t>(), no, m, h->rc_oq.as<int32_t>(),
                            (int32_t)h->r_rules.size(), sorted ? h->rc_okey.as<int32_t>() : nullptr, nullptr, nkeys, 0,
                            &AD, &T, h->a_scratch.p, st, &ag_pk, &ag_fin))
                return rules_step_fail(h, SH_E_HIP, "carried aggregate launch failed");
        }
        // `having`, then the event limiters on the rows it kept, from each run's carried
        // counter: the rows handed to the host queue are the last pass's, from its own
        // buffers (the limiters key the kept rows, so their keys move with them; the
        // aggregates' table below takes every row's state, and the counters' moves last)
        post.step = true;
        post.src = shw_rows{h->w_oseq.as<uint64_t>(), h->w_ovals.as<int64_t>(), h->rc_oq.as<int32_t>(),
                            h->rc_ots.as<int64_t>(), nullptr, rl_keyed ? h->rc_okey.as<int32_t>() : nullptr};
        post.m = m;
        post.n_out = no;
        post.mid = &h->hv;
        post.n_keys = nkeys;
        post.tab = &h->rl_tab;
        const int xrc = row_post(h, post);
        if (xrc) return xrc;
        ml = post.after_having;
        mk = post.after_rate;
    } else {
        hipEventRecord(h->ev[2], st);
    }
    if (shr_carry_rows(scnt, soff, n, lid, blk_off, A.ts.as<int64_t>(), A.key.as<int32_t>(), A.seq.as<uint64_t>(),
                       Bn.ts.as<int64_t>(), Bn.key.as<int32_t>(), Bn.seq.as<uint64_t>(), Bn.c_off.as<uint32_t>(), na,
                       colp, cdst, cw, st))
        return rules_step_fail(h, SH_E_HIP, "rule carry launch failed");
    // rows into the host output queue; the per-key last timestamps move last, when
    // nothing can refuse the step any more
    const size_t base = h->o_seq.size();
    out_queue_rows(h, base + mk);
    if (mk > 0) {
        const shw_rows& o = post.out;
        hipMemcpyAsync(h->o_query.data() + base, o.query, (size_t)mk * 4, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(h->o_seq.data() + base, o.seq, (size_t)mk * 8, hipMemcpyDeviceToHost, st);
        hipMemcpyAsync(h->o_ts.data() + base, o.ts, (size_t)mk * 8, hipMemcpyDeviceToHost, st);
        if (h->n_out)
            hipMemcpyAsync(h->o_vals.data() + base * h->n_out, o.vals, (size_t)mk * h->n_out * 8,
                           hipMemcpyDeviceToHost, st);
    }
    // ... and with them the segments' final aggregate states into their table
    uint64_t ag_ctl[2] = {0, 0};  // entries, error word
    int arc = 0;
    if (ag_pk) {
        const shq_table T = carry_table(h->ag_tab);
        // (the device counter counts this launch alone: every shc_put starts it from zero)
        const DevBuf& ctl = h->ag_tab.ctl;
        hipMemsetAsync(ctl.p, 0, 16, st);
        arc = shc_put(&T, ag_pk, ag_fin, m, ctl.as<unsigned long long>(), ctl.as<int32_t>() + 2, st);
        hipMemcpyAsync(ag_ctl, ctl.p, 16, hipMemcpyDeviceToHost, st);
    }
    // ... and the limiters' next counters into theirs
    uint64_t rl_ctl[2] = {0, 0};
    if (post.put_keys && !arc) {
        const shq_table T = carry_table(h->rl_tab);
        const DevBuf& ctl = h->rl_tab.ctl;
        hipMemsetAsync(ctl.p, 0, 16, st);
        arc = shc_put(&T, post.put_keys, post.put_state, ml, ctl.as<unsigned long long>(), ctl.as<int32_t>() + 2, st);
        hipMemcpyAsync(rl_ctl, ctl.p, 16, hipMemcpyDeviceToHost, st);
    }
    if (shr_klast_update(sts, skeys, perm, n, (uint32_t)nc, h->rc_klast.as<int64_t>(), st) || arc ||
        (hipEventRecord(h->ev[3], st), hipStreamSynchronize(st)) != hipSuccess || (ag_ctl[1] & 1) ||
        (rl_ctl[1] & 1)) {
        out_queue_rows(h, base);
        return rules_step_fail(h, SH_E_HIP, "device error in the rule step");
    }
    phase_times(h);
    h->rc_cur = 1 - h->rc_cur;
    h->rc_rows = nrows;
    h->rc_pairs = npairs;
    h->rc_steps++;
    h->rs_last = 0;
    if (ag_pk) h->ag_tab.entries += (int64_t)ag_ctl[0];  // the slots this step claimed
    if (h->r_aggp) h->agg_last = 6;
    h->hv.last = h->hv_on ? 1 : 0;
    h->hv.rows_in = m;
    h->hv.rows_kept = ml;
    if (post.put_keys) h->rl_tab.entries += (int64_t)rl_ctl[0];
    h->rl.last = h->rl_on ? 1 : 0;
    h->rl.rows_in = ml;
    h->rl.rows_kept = mk;
    rules_unstage(h);
    return SH_OK;
}

shd_batch device_batch(const sh_handle* h, const sh_device_run* run) {
    return shd_batch{run->d_ts, nullptr, nullptr, h->partitioned ? run->d_keys : nullptr, 0, 0, 0, run->n};
}

// the four phase times of sh_kernel_times from the events ev[0..3]
void phase_times(sh_handle* h) {
    hipEventElapsedTime(&h->times.segment_ms, h->ev[0], h->ev[1]);
    hipEventElapsedTime(&h->times.advance_ms, h->ev[1], h->ev[2]);
    hipEventElapsedTime(&h->times.emit_ms, h->ev[2], h->ev[3]);
    hipEventElapsedTime(&h->times.total_ms, h->ev[0], h->ev[3]);
}

// ---- the scaffold of the two bucket-partition engines (run_bucket, run_s3b)

// the plan's shape, and the workspaces and pointers both engines fill; matcher: the
// window matcher's plan (event-sized scan workspace, packed timestamps, the segment
// table), else the sequence carry's. Called after the engine's last "not applicable"
// answer; the staged, match-stream and aggregate columns are the caller's
static int bk_workspace(sh_handle* h, const sh_device_run* run, int kb, bool matcher, const char* oom, shb_plan* B) {
    const int64_t n = run->n;
    B->n = n;
    B->nt = (int32_t)((n + SHB_TILE - 1) / SHB_TILE);
    B->et1 = B->nt;
    B->kb = kb;
    B->no_ts = matcher ? 0 : 1;
    B->tstride = (B->nt + 63) & ~63;
    const int64_t nt = B->nt, slots = nt * SHB_TILE;  // slots: the tiles' bucket order
    if (ensure_ws(h, matcher ? std::max(n, nt + 1) : nt + 1) || h->bk_w0.ensure_fresh(slots * 4) ||
        h->bk_sp.ensure_fresh(n * 2) || h->bk_toff.ensure_fresh(nt * SHB_TOFF * 2) || h->bk_cnt.ensure_fresh(slots) ||
        h->bk_mstart.ensure_fresh(nt * SHB_NB * 4) || h->bk_tpre.ensure_fresh(nt * 8) ||
        h->bk_tfirst.ensure_fresh(nt * 8) || h->bk_hstart.ensure_fresh(nt * 4) ||
        h->bk_ttot.ensure_fresh((nt + 1) * 4) || h->bk_flag.ensure_fresh(64) || h->bk_rd.ensure(64) ||
        h->bk_tofft.ensure_fresh((int64_t)(SHB_NB + 1) * B->tstride * 2) ||
        // the matcher's segment table: each bucket's segment lengths summed over the tiles,
        // written once per step by the partition (12.5 MB at 100M events)
        (matcher && (h->bk_tpfx.ensure_fresh((int64_t)SHB_NB * B->tstride * 4) ||
                     h->bk_tpfb.ensure_fresh((int64_t)SHB_NB * (B->tstride / 64 + 1) * 4))))
        return fail(h, SH_E_OOM, oom);
    B->ts = run->d_ts;
    B->keys = run->d_keys;
    B->w0 = h->bk_w0.as<uint32_t>();
    B->sp = h->bk_sp.as<uint16_t>();
    B->toff = h->bk_toff.as<uint16_t>();
    B->tofft = h->bk_tofft.as<uint16_t>();
    B->tpfx = matcher ? h->bk_tpfx.as<uint32_t>() : nullptr;
    B->tpfb = matcher ? h->bk_tpfb.as<uint32_t>() : nullptr;
    B->cnt = h->bk_cnt.as<uint8_t>();
    B->mstart = h->bk_mstart.as<uint32_t>();
    B->tpre = h->bk_tpre.as<int64_t>();
    B->tfirst = h->bk_tfirst.as<int64_t>();
    B->hstart = h->bk_hstart.as<int32_t>();
    B->ttot = h->bk_ttot.as<uint32_t>();
    B->flag = h->bk_flag.as<int32_t>();
    B->ms_ctr = h->bk_flag.as<uint32_t>() + 4;
    if (shj_bucket_profiled()) {
        if (h->bk_prof.ensure_fresh(128)) return fail(h, SH_E_OOM, "profile");
        hipMemsetAsync(h->bk_prof.p, 0, 128, h->stream);
        B->prof = h->bk_prof.as<unsigned long long>();
    }
    return SH_OK;
}

// ev[0], the flag and total words cleared, the tile-local bucket partition, ev[1]
static int bk_begin(sh_handle* h, const sh_device_run* run, int32_t nkeys, shb_plan* B, const char* what) {
    hipStream_t st = h->stream;
    hipEventRecord(h->ev[0], st);
    hipMemsetAsync(B->flag, 0, 32, st);  // flag word + match-stream allocator
    hipMemsetAsync(B->ttot, 0, ((int64_t)B->nt + 1) * 4, st);
    if (shb_partition(run->d_keys, run->d_ts, nkeys, B, st)) return fail(h, SH_E_HIP, what);
    hipEventRecord(h->ev[1], st);
    return SH_OK;
}

// ev[3] and the read-back of the device's flag word and match total
static int bk_end(sh_handle* h, const shb_plan* B, const char* what, int32_t* flag, int64_t* total) {
    hipStream_t st = h->stream;
    hipEventRecord(h->ev[3], st);
    hipMemcpyAsync(h->bk_rd.as<void>(0), B->flag, 4, hipMemcpyDeviceToHost, st);
    hipMemcpyAsync(h->bk_rd.as<void>(8), B->ttot + B->nt, 4, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, what);
    *flag = *h->bk_rd.as<int32_t>(0);
    *total = *h->bk_rd.as<uint32_t>(8);
    return SH_OK;
}

// the engines' common answer once the caller has judged its own flag bits: a bad key
// id, 1 for any other premise that failed on the device, the match count against the
// capacity, the phase times; *last = 1 (bk_last / s3b_last) when the rows stand
static int bk_close(sh_handle* h, sh_device_run* run, int32_t flag, int64_t total, int* last, const char* what) {
    hipStream_t st = h->stream;
    if (flag & SHB_F_KEY) return fail(h, SH_E_INVALID_ARG, "partition key id >= n_keys");
    if (flag) return 1;
    run->out_count = total;
    if (total > run->out_capacity) return fail(h, SH_E_MORE, "output capacity too small");
    if (run->d_out_query && total > 0) hipMemsetAsync(run->d_out_query, 0, total * 4, st);
    phase_times(h);
    h->times.advance_launches = 1;
    *last = 1;
    return hipStreamSynchronize(st) == hipSuccess ? SH_OK : fail(h, SH_E_HIP, what);
}

// The emitter of a run's select list and layout: the kernel hipRTC compiles for them
// (sh_jit.cpp gen_emit; compiled at the first run of a layout, kept on the handle), or
// nullptr for the generic k_bk_emit: lists of more than 8 values, a failed compile, and
// SH_BK_EMIT_SPEC=0 (read per call). Sets bk_emit_last
static void* bk_emit_fn(sh_handle* h, const shb_out& O, const shb_cols& OC) {
    h->bk_emit_last = 0;
    if (const char* e = getenv("SH_BK_EMIT_SPEC"))
        if (atoi(e) == 0) return nullptr;
    shj_emit_key K;
    if (shj_emit_key_of(&O, &OC, &K)) return nullptr;
    const sh_handle::BkEmit* hit = nullptr;
    for (const auto& c : h->bk_emit)
        if (!memcmp(&c.key, &K, sizeof(K))) hit = &c;
    if (!hit) {
        void* fn = nullptr;
        if (shj_emit_load(&K, &fn, &h->bk_emit_err)) fn = nullptr;
        h->bk_emit.push_back({K, fn});
        hit = &h->bk_emit.back();
    }
    h->bk_emit_last = hit->fn ? 1 : -1;
    return hit->fn;
}

static int bk_emit(void* fn, const shb_plan& B, const shb_out& O, const shb_cols& OC, sh_device_run* run,
                   hipStream_t stream) {
    return fn ? shb_emit_spec(fn, &B, &O, &OC, 0, run->d_out_seq, run->d_out_values, run->out_capacity, stream)
              : shb_emit(&B, &O, &OC, 0, run->d_out_seq, run->d_out_values, run->out_capacity, stream);
}

// chunks per time segment of run_bucket's matcher / emitter pipeline (C2: 8 chunks 3.90 ms
// per step, 16 3.70, 32 3.66-3.68 against the single launch's 3.70-3.74,
// profiles/c2_pipeline_ab.txt)
static constexpr int SH_BK_SEG_CHUNKS = 32;

// run_bucket's launches between the partition (ev[1]) and the read-back: the matcher,
// the carry of the aggregates (AG, or nullptr), the scans and the emitter; ev[2] is
// recorded between the matchers and the emitters' tail
static int bucket_launch(sh_handle* h, sh_device_run* run, shb_plan& B, const shb_out& O, const shb_cols& OC,
                         const shb_aggc* AG) {
    hipStream_t st = h->stream;
    void* args[] = {&B};
    void* const efn = bk_emit_fn(h, O, OC);
    // The matcher (VALU and LDS bound) and the emitter (parked on memory) overlap over
    // time segments of whole chunks: the matchers of segment 0, 1, ... on the caller's
    // stream, an event after each; behind that event, on the handle's side stream, the
    // segment's carry scan and emitter. An emitter workgroup reads cnt, mstart and ttot
    // of its own tile, which the matcher workgroups of that tile's chunk alone write
    // (halo tiles are read only), and its first row: the running total the carry scan
    // hands on. Aggregate carries, the phase clocks and steps shorter than two segments
    // keep the single launch. SH_BK_SEG: chunks per segment (0: single launch), read per
    // call (profiles/c2_pipeline_ab.txt)
    int seg = SH_BK_SEG_CHUNKS;
    if (const char* e = getenv("SH_BK_SEG")) seg = atoi(e);
    if (seg > 0) seg = std::max(seg, (B.n_chunks + sh_handle::SH_BK_SEGS - 1) / sh_handle::SH_BK_SEGS);
    const int n_seg = seg > 0 ? (B.n_chunks + seg - 1) / seg : 1;
    const bool piped = !AG && !B.prof && (n_seg >= 2 || (seg > 0 && getenv("SH_BK_SEG")));
    if (piped && !h->bk_side) {
        // (created with the highest priority it lost: 3.706 against 3.682 ms per step)
        if (hipStreamCreateWithFlags(&h->bk_side, hipStreamNonBlocking) != hipSuccess) {
            h->bk_side = nullptr;
            return fail(h, SH_E_HIP, "bucket side stream");
        }
    }
    for (auto& e : h->bk_ev)
        if (piped && !e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            e = nullptr;
            return fail(h, SH_E_HIP, "bucket events");
        }
    if (piped) {
        hipStream_t sd = h->bk_side;
        // (a failed launch leaves by way of both streams: the fallback engines write the
        // same output buffers)
        auto quit = [&](const char* what) {
            hipStreamSynchronize(sd);
            hipStreamSynchronize(st);
            return fail(h, SH_E_HIP, what);
        };
        for (int k = 0; k < n_seg; k++) {
            const int c0 = k * seg, c1 = std::min(c0 + seg, B.n_chunks);
            B.c0 = c0;
            B.et0 = c0 * B.ct;
            B.et1 = std::min(c1 * B.ct, B.nt);
            if (hipModuleLaunchKernel((hipFunction_t)h->bk.match, (unsigned)(SHB_NB * (c1 - c0)), 1, 1, 512, 1, 1, 0, st,
                                      args, nullptr) != hipSuccess)
                return quit("shb_match launch failed");
            if (hipEventRecord(h->bk_ev[k], st) != hipSuccess || hipStreamWaitEvent(sd, h->bk_ev[k], 0) != hipSuccess)
                return quit("bucket segment event");
            if (shb_finish_seg(&B, B.et0, B.et1, B.ms_ctr + 2, k == n_seg - 1, sd)) return quit("bucket scan launch failed");
            if (bk_emit(efn, B, O, OC, run, sd))
                return quit("bucket emit launch failed");
        }
        // advance_ms: the matchers (and what of the emitters ran beside them); emit_ms:
        // the emitters' tail after the last matcher segment
        hipEventRecord(h->ev[2], st);
        if (hipEventRecord(h->bk_ev[sh_handle::SH_BK_SEGS], sd) != hipSuccess ||
            hipStreamWaitEvent(st, h->bk_ev[sh_handle::SH_BK_SEGS], 0) != hipSuccess)
            return quit("bucket join event");
    } else {
        if (hipModuleLaunchKernel((hipFunction_t)h->bk.match, (unsigned)(SHB_NB * B.n_chunks), 1, 1, 512, 1, 1, 0, st,
                                  args, nullptr) != hipSuccess)
            return fail(h, SH_E_HIP, "shb_match launch failed");
        if (AG && shb_agg_carry(&B, AG, st)) return fail(h, SH_E_HIP, "aggregate carry launch failed");
        if (shb_finish(&B, h->w_scan.as<uint32_t>(), st)) return fail(h, SH_E_HIP, "bucket scan launch failed");
        hipEventRecord(h->ev[2], st);
        if (bk_emit(efn, B, O, OC, run, st)) return fail(h, SH_E_HIP, "bucket emit launch failed");
    }
    return SH_OK;
}

// bucketed window engine (sh_bucket.hip): partitioned window programs with a
// consumer-side form and a null-free projection; 0 ok, 1 = not applicable or a
// premise failed on the device (the caller runs the general window path),
// SH_E_MORE = output capacity too small (out_count = matches), <0 error.
// mode: how an aggregating select's running values are formed; a select the carry
// plan does not take leaves the arguments in the rows whatever the mode (res->carried
// says which), and the device's refusal of the parallel carry answers 1 with
// res->refused: the caller runs the next mode
int run_bucket(sh_handle* h, sh_device_run* run, int32_t nkeys, BkAgg mode, BkRun* res) {
    static const bool off = getenv("SH_DISABLE_BUCKET") != nullptr;
    h->bk_last = 0;
    h->bk_emit_last = 0;
    *res = BkRun{};
    const shp_program& P = h->prog;
    const int64_t n = run->n;
    if (off || !h->partitioned || nkeys < 1024 || !P.out_fast || n < SHB_TILE) return 1;
    // a max / min select is not offered to this engine yet: the window engine writes
    // its arguments and the post-pass (sh_agg.hip "max / min") forms the values
    for (int o = 0; o < P.n_out; o++)
        if (P.out_agg[o] == SH_AGG_MAX || P.out_agg[o] == SH_AGG_MIN) return 1;
    const int kb = std::max(0, bits_for((uint64_t)(nkeys - 1)) - 8);
    if (kb > 8) return 1;
    shb_out O;
    shb_select S;
    if (shb_plan_select(P, h->part_attr0, run->d_cols, &O, &S)) return 1;
    if (h->bk_state == 0) {
        const int lrc = shj_bucket_load(&P, S.ms, S.n_ms, &h->bk, &h->bk_err);
        h->bk_state = lrc == 0 ? 1 : (lrc == -1 ? -2 : -1);  // -2: no consumer-side form (not applicable)
    }
    if (h->bk_state != 1) return 1;
    if (n >= ((int64_t)1 << 32) - SHB_TILE) return 1;  // event indices are 32-bit on this engine
    shb_plan B{};
    B.n_staged = h->bk.n_staged;
    for (int k = 0; k < B.n_staged; k++) {
        B.st_src[k] = run->d_cols[h->bk.staged_attr[k]];
        B.st_width[k] = type_width(P.attr_type[0][h->bk.staged_attr[k]]);
    }
    // k_bk_aggp (the additions as a segmented prefix, exact in 64-bit fixed point, refused
    // on the device by a value that is not) or k_bk_aggc (the reference's own additions,
    // no exactness proof; every key of a bucket walked in one workgroup: C2's 40 keys per
    // bucket leave most lanes idle -- 28 ms against the post-pass's 8.7)
    // (the running values go by match-stream position; by output row, through a per-slot
    // row map, measured 8.39 vs 7.65 ms/step in round 5: removed)
    shb_aggc AG{};
    int agg_of[SHB_MAX_OUT];
    bool carry = P.agg_post && mode != BK_AGG_ROWS;
    if (carry) {
        const shb_carry_plan cp = shb_plan_carry(P, run->d_cols, S.ms_of, &B, &AG, agg_of);
        if (cp == SHB_CARRY_NA) return 1;
        carry = cp == SHB_CARRY;
    }
    AG.parallel = mode == BK_AGG_PAR ? 1 : 0;
    // (the post-pass reads raw rows: never written into the caller's packed rows or typed columns)
    if (P.agg_post && !carry && h->out_mode != SHB_OUT_RAW && !h->cols_rows) return 1;
    // every pointer below is taken after its buffer's last ensure_fresh
    if (const int wrc = bk_workspace(h, run, kb, true, "bucket workspace", &B)) return wrc;
    // tiles per matcher chunk: 15/16 of the pass's consumer limit in events of a
    // bucket at uniform keys (32 per tile; 60 tiles at 2,048), so a chunk and its
    // halo fit the LDS span; denser buckets split (C2: 60 tiles 1.90 ms, 56 1.97-1.99,
    // 52 2.07, 64 2.50 in one call, profiles/r6_c2_ct_ab.txt)
    static const int ct_env = getenv("SH_BK_CT") ? atoi(getenv("SH_BK_CT")) : 0;
    B.ct = ct_env > 0 ? std::min(ct_env, SHB_CT_MAX) : std::min(shj_bucket_chunk() * 15 / 512, SHB_CT_MAX);
    B.n_chunks = (B.nt + B.ct - 1) / B.ct;
    B.within = std::max<int64_t>(0, P.within_ms);
    for (int k = 0; k < B.n_staged; k++) {
        if (h->bk_st[k].ensure_fresh((int64_t)B.nt * SHB_TILE * B.st_width[k])) return fail(h, SH_E_OOM, "bucket workspace");
        B.st_dst[k] = h->bk_st[k].p;
    }
    // match stream: one region of SHB_SPAN values per matcher workgroup (its first
    // pass), then a shared tail for further passes; every partial is consumed at
    // most once, so n values suffice for the tail
    B.n_ms = S.n_ms;
    const int64_t ms_vals = (int64_t)SHB_NB * B.n_chunks * SHB_SPAN + n;
    for (int m = 0; m < S.n_ms; m++) {
        B.ms_width[m] = type_width(P.attr_type[0][S.ms[m]]);
        if (h->bk_ms[m].ensure_fresh(ms_vals * B.ms_width[m])) return fail(h, SH_E_OOM, "match stream");
        B.ms[m] = h->bk_ms[m].p;
    }
    for (int i = 0; carry && i < AG.n; i++) {
        if (h->bk_agg[i].ensure_fresh(ms_vals * 8)) return fail(h, SH_E_OOM, "aggregate columns");
        AG.out[i] = h->bk_agg[i].p;
    }
    for (int o = 0; o < O.n_out; o++) {
        if (S.ms_of[o] >= 0) O.src[o] = B.ms[S.ms_of[o]];
        if (carry && agg_of[o] >= 0) {
            O.kind[o] = 0;
            O.src[o] = AG.out[agg_of[o]];
            O.type[o] = P.out_type[o];
        }
    }
    shb_cols OC{};
    if (!P.agg_post || carry) {
        int32_t wd[SHB_MAX_OUT];
        for (int o = 0; o < O.n_out; o++) wd[o] = type_width(O.type[o]);
        direct_layout(h, run, wd, O.n_out, &OC);
    }
    // packed timestamps: ts - tbase in 32 - kb bits, centred on the first event
    hipStream_t st = h->stream;
    hipMemcpyAsync(h->bk_rd.p, run->d_ts, 8, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "bucket: timestamp read");
    B.tbase = *h->bk_rd.as<int64_t>() - ((int64_t)1 << (31 - kb));
    if (const int brc = bk_begin(h, run, nkeys, &B, "bucket partition launch failed")) return brc;
    if (const int lrc = bucket_launch(h, run, B, O, OC, carry ? &AG : nullptr)) return lrc;
    int32_t flag = 0;
    int64_t total = 0;
    if (const int erc = bk_end(h, &B, "device error in bucket engine", &flag, &total)) return erc;
    if (B.prof) {
        unsigned long long pr[16];
        hipMemcpy(pr, B.prof, 128, hipMemcpyDeviceToHost);
        fprintf(stderr, "[shb_match clock ticks, sum over workgroups] table %llu load %llu rank %llu walk %llu "
                        "scan+psum %llu emit %llu\n",
                pr[5], pr[0], pr[1], pr[2], pr[3], pr[4]);
        if (carry && AG.parallel)
            fprintf(stderr, "[k_bk_aggp clock ticks, sum over workgroups] table+load %llu sort %llu rows %llu "
                            "scans %llu\n",
                    pr[8], pr[9], pr[10], pr[11]);
        else if (carry)
            fprintf(stderr, "[k_bk_aggc clock ticks, sum over workgroups] table %llu load+prefix %llu e1 %llu "
                            "sort %llu walk %llu\n",
                    pr[8], pr[9], pr[10], pr[11], pr[12]);
    }
    if (flag == SHB_F_AGG && carry && AG.parallel) {
        // a value the fixed point cannot hold exactly (or a chunk too dense): the batch
        // again in the caller's next mode, the post-pass adding instead. The refusal
        // sticks to the handle: data that fails the fixed-point test once (a price such
        // as 12.34) fails it in every batch, and each refused attempt costs a whole
        // bucketed pipeline
        h->aggp_refused = res->refused = true;
        return 1;
    }
    const int rc = bk_close(h, run, flag, total, &h->bk_last, "bucket engine");
    if (h->bk_last && carry) {
        res->carried = mode;
        h->agg_last = AG.parallel ? 5 : 4;
    }
    return rc;
}

// the rise-and-fall sequence on the bucket-carry engine (sh_bucket.hip k_s3b):
// the tile-local bucket partition, one workgroup per bucket carrying its keys'
// state across the stream, the ordered rows by k_bk_emit. 0 ok, 1 = not
// applicable or refused on the device (the caller runs k_seq3s), <0 error
int run_s3b(sh_handle* h, sh_device_run* run, int32_t nkeys) {
    const bool off = getenv("SH_DISABLE_S3B") != nullptr || getenv("SH_NO_SEQ3") != nullptr;  // (per call: tests A/B it)
    h->s3b_last = 0;
    h->bk_emit_last = 0;
    const nf_query& Q = nf_bulk_table(h)->q[0];
    if (off || !h->partitioned || h->T->n_queries != 1 || !Q.s3 || nkeys < 1024 || run->n < SHB_TILE) return 1;
    const int kb = std::max(0, bits_for((uint64_t)(nkeys - 1)) - 8);
    if (kb > 12 || Q.contains_agg) return 1;
    // every operand and select value: one 4-byte attribute A (no null masks on this path)
    const int A = Q.s3_a2, ty = Q.s3_t2;
    if (!(ty == SH_T_FLOAT || ty == SH_T_INT) || A < 0 || A >= (int)h->stream_types[0].size() ||
        type_width(h->stream_types[0][A]) != 4 || Q.s3_a3 != A || Q.s3_e1a != A || Q.s3_la != A || Q.s3_t3 != ty ||
        Q.s3_e1t != ty || Q.s3_lt != ty)
        return 1;
    shb_out O{};
    O.n_out = Q.n_out;
    shb_s3 S{};
    S.type = ty;
    S.warm = 1;  // (the next chunk's gather overlaps the walk: 3.42 vs 3.52 ms, profiles/r4_c3_s3b_warm_ab.txt)
    S.op2 = Q.s3_op2;
    S.dom2 = Q.s3_dom2;
    S.op3 = Q.s3_op3;
    S.dom3 = Q.s3_dom3;
    int ms_of[SHB_MAX_OUT];
    for (int o = 0; o < Q.n_out; o++) {
        if (Q.s3_out_attr[o] != A || Q.s3_out_type[o] != ty) return 1;
        O.type[o] = ty;
        ms_of[o] = -1;
        const int sl = Q.s3_out_slot[o];
        if (sl == 2) {
            O.kind[o] = 1;
            O.src[o] = run->d_cols[A];
            continue;
        }
        int m = 0;
        while (m < S.n_ms && S.ms_slot[m] != sl) m++;
        if (m == S.n_ms) S.ms_slot[S.n_ms++] = sl;
        O.kind[o] = 0;
        ms_of[o] = m;
    }
    shb_plan B{};
    if (const int wrc = bk_workspace(h, run, kb, false, "sequence workspace", &B)) return wrc;
    const int64_t slots = (int64_t)B.nt * SHB_TILE;
    if (h->bk_st[0].ensure_fresh(slots * 4)) return fail(h, SH_E_OOM, "sequence workspace");
    B.n_staged = 1;
    B.st_src[0] = run->d_cols[A];
    B.st_dst[0] = h->bk_st[0].p;
    B.st_width[0] = 4;
    // match stream: at most one match per event, in its segment's slots
    B.n_ms = S.n_ms;
    for (int m = 0; m < S.n_ms; m++) {
        if (h->bk_ms[m].ensure_fresh(slots * 4)) return fail(h, SH_E_OOM, "match stream");
        B.ms[m] = h->bk_ms[m].p;
        B.ms_width[m] = 4;
    }
    for (int o = 0; o < O.n_out; o++)
        if (ms_of[o] >= 0) O.src[o] = B.ms[ms_of[o]];
    shb_cols OC;
    int32_t wd[SHB_MAX_OUT];
    for (int o = 0; o < O.n_out; o++) wd[o] = 4;
    direct_layout(h, run, wd, O.n_out, &OC);
    hipStream_t st = h->stream;
    if (const int brc = bk_begin(h, run, nkeys, &B, "sequence partition failed")) return brc;
    if (shb_s3_carry(&B, &S, st)) return fail(h, SH_E_HIP, "sequence carry launch failed");
    if (shb_finish(&B, h->w_scan.as<uint32_t>(), st)) return fail(h, SH_E_HIP, "sequence scan failed");
    hipEventRecord(h->ev[2], st);
    if (bk_emit(bk_emit_fn(h, O, OC), B, O, OC, run, st)) return fail(h, SH_E_HIP, "sequence emit failed");
    int32_t flag = 0;
    int64_t total = 0;
    if (const int erc = bk_end(h, &B, "device error in the sequence engine", &flag, &total)) return erc;
    if (B.prof) {
        unsigned long long pr[16];
        hipMemcpy(pr, B.prof, 128, hipMemcpyDeviceToHost);
        fprintf(stderr, "[k_s3b clock ticks, sum over workgroups] tables+load %llu sort %llu carry %llu out %llu\n",
                pr[0], pr[1], pr[2], pr[3]);
    }
    return bk_close(h, run, flag, total, &h->s3b_last, "sequence engine");
}

// the window engine (sh_window.hip): the key segments, the matcher over each key's
// events and the ordered placement; rows and sequence numbers are raw (a caller's
// other layout is converted afterwards). 0 ok, 1 = not applicable (more than 7
// attributes) or timestamps decrease inside a key (the caller runs the sequential
// per-key engine), SH_E_MORE = output capacity too small, <0 error
int run_window(sh_handle* h, sh_device_run* run, int32_t nkeys) {
    if (h->stream_types[0].size() > 7) return 1;
    const shd_batch B = device_batch(h, run);
    int64_t nm = 0;
    const int64_t n = run->n;
    hipStream_t st = h->stream;
    if (ensure_ws(h, n)) return fail(h, SH_E_OOM, "workspace");
    const int na = (int)h->stream_types[0].size();
    const bool sorted = h->partitioned;  // unpartitioned: one segment, arrival order
    shd_window_ws wws{};
    if (h->v_mpos.ensure_fresh(n * 4) || h->v_flag.ensure_fresh(64) || h->v_cnts.ensure_fresh(n * 4))
        return fail(h, SH_E_OOM, "window workspace");
    shd_payload carry;
    void* mid[8] = {nullptr};
    int alias = -1;
    if (sorted && carry_setup(h, run, &carry, mid, &alias)) return fail(h, SH_E_OOM, "window workspace");
    wws.match_pos = h->v_mpos.as<int32_t>();
    wws.cnt_s = h->v_cnts.as<uint32_t>();
    wws.cnt = h->w_cnt.as<uint32_t>();
    wws.off = h->w_off.as<uint32_t>();
    wws.flag = h->v_flag.as<int32_t>();
    // arrival tiles: the sorted order becomes (tile, key, arrival), so the
    // count scatter and the ordered placement touch one tile's output window
    // at a time (L2 / Infinity-Cache resident) instead of the whole stream
    const int tshift = sorted ? tile_shift_for(n, nkeys) : 0;
    hipEventRecord(h->ev[0], st);
    shd_segment_ws ws = seg_ws(h, n);
    const uint32_t* perm = nullptr;
    const uint32_t* skeys = nullptr;
    if (shd_segment_payload(&B, nkeys, &ws, st, &perm, &skeys, sorted ? &carry : nullptr, mid, tshift, 0))
        return fail(h, SH_E_HIP, "segment launch failed");
    shd_tiles TL{};
    if (tshift) {
        TL.K1 = (uint32_t)nkeys + 1;
        TL.ntile = (uint32_t)((n + ((int64_t)1 << tshift) - 1) >> tshift);
        TL.shift = tshift;
        const size_t words = (size_t)TL.ntile * TL.K1;
        if (h->v_dir.ensure_fresh(words * 8)) return fail(h, SH_E_OOM, "tile directory");
        TL.dstart = h->v_dir.as<uint32_t>();
        TL.dend = h->v_dir.as<uint32_t>() + words;
        if (shd_tile_dir(skeys, n, tshift, TL.K1, TL.ntile, (uint32_t*)TL.dstart, (uint32_t*)TL.dend, st))
            return fail(h, SH_E_HIP, "tile directory launch failed");
    }
    hipEventRecord(h->ev[1], st);
    const int64_t* sts = sorted ? h->v_sts.as<int64_t>() : run->d_ts;
    const void* scols[32];
    for (int a = 0; a < na; a++) scols[a] = sorted ? (const void*)h->v_scol[a].p : run->d_cols[a];
    if (alias >= 0) scols[alias] = skeys;  // the partition column in key-segment order is the sorted key
    if (h->jit_state == 0) {
        if (getenv("SH_DISABLE_JIT")) {
            h->jit_state = -1;
            h->jit_err = "disabled by SH_DISABLE_JIT";
        } else {
            h->jit_state = shj_window_load(&h->prog, &h->jit, &h->jit_err) == 0 ? 1 : -1;
        }
    }
    int wrc = shd_window(h->d_prog.as<shp_program>(), &h->prog, &B, nkeys, perm, skeys, sts, scols, &wws,
                         h->d_cols_desc.as<shd_cols>(), h->w_scan.as<uint32_t>(), run->d_out_seq, nullptr,
                         run->d_out_values, nullptr, run->out_capacity, &nm, st, h->ev[2],
                         h->jit_state == 1 ? &h->jit : nullptr, tshift ? &TL : nullptr);
    hipEventRecord(h->ev[3], st);
    if (hipStreamSynchronize(st) != hipSuccess) return fail(h, SH_E_HIP, "device error in window engine");
    if (wrc < 0) return fail(h, SH_E_HIP, "window engine launch failed");
    run->out_count = nm;
    if (wrc == 2) return fail(h, SH_E_MORE, "output capacity too small");
    if (wrc == 1) return 1;  // timestamps decrease inside a key
    if (run->d_out_query && nm > 0) hipMemsetAsync(run->d_out_query, 0, nm * 4, st);
    phase_times(h);
    h->times.advance_launches = 1;
    return SH_OK;
}

// typed output columns requested: engines that write raw rows write them into a
// workspace that sh_run_device narrows afterwards (the bucketed engine writes
// the columns itself)
int rows_for_cols(sh_handle* h, sh_device_run* run) {
    if (h->out_mode == SHB_OUT_RAW || h->cols_rows) return SH_OK;
    const size_t cap = (size_t)std::max<int64_t>(1, run->out_capacity);
    if (h->w_colrows.ensure(cap * std::max(1, h->n_out) * 8)) return fail(h, SH_E_OOM, "typed-column row workspace");
    run->d_out_values = h->w_colrows.as<int64_t>();
    if (h->out_mode == SHB_OUT_PACKED) {
        if (h->w_packseq.ensure(cap * 8)) return fail(h, SH_E_OOM, "packed-row workspace");
        run->d_out_seq = h->w_packseq.as<uint64_t>();
    }
    h->cols_rows = true;
    return SH_OK;
}

void direct_layout(sh_handle* h, sh_device_run* run, const int32_t* widths, int n_out, shb_cols* OC) {
    memset(OC, 0, sizeof(*OC));
    if (h->out_mode == SHB_OUT_RAW || h->cols_rows) return;
    OC->use = h->out_mode;
    for (int o = 0; o < n_out && o < SHB_MAX_OUT; o++) {
        OC->colw[o] = h->out_mode == SHB_OUT_PACKED ? h->pk_w[o] : widths[o];
        if (h->out_mode == SHB_OUT_COLS) OC->cols[o] = run->d_out_cols[o];
        else OC->woff[o] = h->pk_woff[o];
    }
    if (h->out_mode == SHB_OUT_PACKED) {
        OC->rw = h->pk_rw;
        OC->rows = run->d_out_values;
    }
}

// the running aggregates of the fast engines' ordered rows (sh_agg.hip): SH_OK,
// 1 = the double additions would round (the caller reruns sequentially), < 0 error
int agg_post(sh_handle* h, sh_device_run* run, int32_t nkeys, const int32_t* d_query, int n_query,
                    const int32_t* agg_kind, const int32_t* arg_type, int n_out) {
    const int64_t m = run->out_count;
    if (m <= 0) return SH_OK;
    sha_desc D;
    memset(&D, 0, sizeof(D));
    for (int o = 0; o < n_out && D.n_cols < SHA_MAX_COLS; o++)
        if (agg_kind[o] != SH_AGG_NONE) {
            D.c[D.n_cols].col = o;
            D.c[D.n_cols].kind = agg_kind[o];
            D.c[D.n_cols].arg_type = arg_type[o];
            D.n_cols++;
        }
    if (D.n_cols == 0) return SH_OK;
    // under `group by` (h->grp_on: a chain-mode query or a small rule set) the segments
    // are (query, key, group values)
    const bool grouped = h->grp_on;
    if (h->a_scratch.ensure((size_t)(grouped ? sha_grouped_scratch_bytes(m, D.n_cols) : sha_scratch_bytes(m, D.n_cols))))
        return fail(h, SH_E_OOM, "aggregate scratch");
    hipEventRecord(h->ev[4], h->stream);
    const int32_t* keys = h->partitioned ? run->d_keys : nullptr;
    const int32_t nk = h->partitioned ? nkeys : 1;
    const int rc = grouped ? sha_running_grouped(run->d_out_seq, run->d_out_values, n_out, m, d_query, n_query, keys, nk,
                                                 0, &D, &h->grp, h->a_scratch.p, h->stream)
                           : sha_running(run->d_out_seq, run->d_out_values, n_out, m, d_query, n_query, keys, nk, 0, &D,
                                         h->a_scratch.p, h->stream);
    h->grp_last = grouped && rc == 0 ? 1 : 0;
    if (rc < 0) return fail(h, SH_E_HIP, "aggregate post-pass failed");
    hipEventRecord(h->ev[5], h->stream);
    if (hipEventSynchronize(h->ev[5]) != hipSuccess) return fail(h, SH_E_HIP, "aggregate post-pass failed");
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->ev[4], h->ev[5]);
    h->times.emit_ms += ms;
    h->times.total_ms += ms;
    h->agg_post_ms = ms;
    h->agg_last = rc == 0 ? 1 : 2;
    return rc;
}
