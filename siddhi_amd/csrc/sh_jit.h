// sh_jit.h — hipRTC specialisation of the window engine (sh_jit.cpp), host side.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "sh_device.h"
#include "sh_program.h"

struct shj_window {
    const void* code;     // gfx950 code object (owned by the process-wide cache)
    size_t code_size;
    void* match;          // hipFunction_t shj_match (after shj_window_load)
    void* place;          // hipFunction_t shj_place
    void* count;          // hipFunction_t shj_count (consumer-side walk), NULL when the filter has no such form
    void* emit;           // hipFunction_t shj_emit
};

// generated source for a window-shaped program (0), -1 if it has no straight-line form
int shj_window_source(const shp_program* hp, std::string* src);
// compile only (no device needed); cached per distinct source for the process
int shj_window_compile(const shp_program* hp, shj_window* out, std::string* err);
// compile + load the module on the current device
int shj_window_load(const shp_program* hp, shj_window* out, std::string* err);
// grid of the XCD-major tile mapping for n events; returns the workgroup count
unsigned shj_tiles(int64_t n, uint32_t* tiles_per_xcd, uint32_t* ntiles);
int shj_tile_size(void);
// the bucketed matcher's consumer limit per pass (events; SH_BK_CH)
int shj_bucket_chunk(void);
// 1 when SH_BK_PROFILE asks for the bucketed matcher's phase clocks (read once per
// process): the generator emits them and the host hands the kernel their buffer
int shj_bucket_profiled(void);

// bucketed window engine matcher (shb_match); ms_attrs: stream attributes the
// match stream carries (e1-side select values), in match-stream column order
struct shj_bucket {
    void* match;          // hipFunction_t shb_match
    int n_staged;         // columns the partition moves into bucket order
    int staged_attr[4];
};
int shj_bucket_load(const shp_program* hp, const int* ms_attrs, int n_ms, shj_bucket* out, std::string* err);
int shj_bucket_source(const shp_program* hp, const int* ms_attrs, int n_ms, std::string* src);
int shj_bucket_compile(const shp_program* hp, const int* ms_attrs, int n_ms, std::string* err);

// bucketed emitter (sh_bk_emit.h) compiled for one select list and output layout: the
// descriptors k_bk_emit reads from its arguments become constants of the kernel.
// Lists of 1 .. SHJ_EMIT_MAX values; longer ones keep the generic kernel
#define SHJ_EMIT_MAX 8
struct shj_emit_key {
    int32_t mode;                  // SHB_OUT_*
    int32_t no;                    // select values
    int32_t rw;                    // packed: words per row
    int32_t kind[SHJ_EMIT_MAX];    // shb_out.kind
    int32_t type[SHJ_EMIT_MAX];    // shb_out.type
    int32_t woff[SHJ_EMIT_MAX];    // packed: shb_cols.woff
    int32_t colw[SHJ_EMIT_MAX];    // packed / typed columns: shb_cols.colw
};
// the key of a launch's descriptors (unused fields zero, so keys compare by memcmp);
// -1: no specialised form (the value count, or a packed row the emitter does not take)
int shj_emit_key_of(const shb_out* O, const shb_cols* OC, shj_emit_key* K);
// occupancy form (waves per SIMD: 6 or 4, as bk_emit_launch chooses it) and rows per lane and round
void shj_emit_form(const shj_emit_key* K, int* occ, int* ru);
// generated source and the kernel's name (no device needed)
int shj_emit_source(const shj_emit_key* K, std::string* src, std::string* name);
int shj_emit_compile(const shj_emit_key* K, std::string* err);
// compile + load on the current device; *fn: hipFunction_t for shb_emit_spec
int shj_emit_load(const shj_emit_key* K, void** fn, std::string* err);
