// prims_layout.cpp — TEST INFRASTRUCTURE: prints the size and every member offset
// of the structures tests/device_prims.py mirrors with ctypes, one
// "struct member offset" line each ("struct sizeof bytes" for the size).
#include <stddef.h>
#include <stdio.h>

#include "../../siddhi_amd/csrc/sh_agg_seq.h"
#include "../../siddhi_amd/csrc/sh_device.h"
#include "../../siddhi_amd/csrc/sh_having.h"

#define SZ(S) printf(#S " sizeof %zu\n", sizeof(S))
#define OFF(S, M) printf(#S " " #M " %zu\n", offsetof(S, M))

int main() {
    SZ(shd_batch);
    OFF(shd_batch, ts);
    OFF(shd_batch, stream);
    OFF(shd_batch, row);
    OFF(shd_batch, keys);
    OFF(shd_batch, row_base);
    OFF(shd_batch, pad);
    OFF(shd_batch, seq_base);
    OFF(shd_batch, n);
    SZ(shd_segment_ws);
    OFF(shd_segment_ws, keys_a);
    OFF(shd_segment_ws, keys_b);
    OFF(shd_segment_ws, idx_a);
    OFF(shd_segment_ws, idx_b);
    OFF(shd_segment_ws, hist);
    OFF(shd_segment_ws, scan_tmp);
    OFF(shd_segment_ws, seg_off);
    OFF(shd_segment_ws, cap);
    SZ(shd_payload);
    OFF(shd_payload, n);
    OFF(shd_payload, pad);
    OFF(shd_payload, src);
    OFF(shd_payload, dst);
    OFF(shd_payload, width);
    SZ(shw_rows);
    OFF(shw_rows, seq);
    OFF(shw_rows, vals);
    OFF(shw_rows, query);
    OFF(shw_rows, ts);
    OFF(shw_rows, nulls);
    OFF(shw_rows, key);
    SZ(shw_rows_out);
    OFF(shw_rows_out, seq);
    OFF(shw_rows_out, vals);
    OFF(shw_rows_out, query);
    OFF(shw_rows_out, ts);
    OFF(shw_rows_out, nulls);
    OFF(shw_rows_out, key);
    SZ(sha_col);
    OFF(sha_col, col);
    OFF(sha_col, kind);
    OFF(sha_col, arg_type);
    OFF(sha_col, pad);
    SZ(sha_desc);
    OFF(sha_desc, n_cols);
    OFF(sha_desc, pad);
    OFF(sha_desc, c);
    SZ(shq_table);
    OFF(shq_table, keys);
    OFF(shq_table, state);
    OFF(shq_table, cap);
    OFF(shq_table, n_cols);
    OFF(shq_table, pad);
    return 0;
}
