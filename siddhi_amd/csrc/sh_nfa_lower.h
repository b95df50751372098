// sh_nfa_lower.h — host lowering of sh_app_desc into the general engine's
// NFA table (sh_nfa_lower.cpp).
#pragma once
#include <string>

#include "sh_nfa.h"

// 0 ok, -1 unsupported (err says why).
// bulk_s3 (or NULL): the caller's row post-filter stage takes the `having` / event limiter
// of a one-query app in bulk runs. The table is lowered exactly as without the stage
// (its selector applies both: streaming, snapshot images and the fingerprint see no
// difference); the s3 fields of *bulk_s3 -- the rest is zero -- say whether the query
// is the rise-and-fall sequence but for those clauses, for sh_run_device's rungs alone
int nf_lower(const sh_app_desc* app, nf_table* T, std::string* err, nf_query* bulk_s3 = nullptr);
// (re)computes every query's per-key layout and the key block size
void nf_set_caps(nf_table* T, int list_cap, int se_cap, int node_cap, int hold_cap, int sched_cap,
                 int group_cap = 4);
