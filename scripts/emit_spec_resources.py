"""Compile-time resources of the bucketed engine's specialised emitters (sh_jit.cpp
gen_emit), from offline hipcc builds of their generated source (no GPU needed): for
each form and each rows-per-lane count asked for, VGPRs, spills, scratch and
occupancy. The rows-per-lane table of shj_emit_form is derived from this output.

    python scripts/emit_spec_resources.py [--ru 1,2,3,4,5,6] [--forms c2,c3,c2agg,c2raw,cases,synthetic]

`--ru 0` compiles each form once, at the rows per lane shj_emit_form gives it."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from siddhi_amd import abi, build  # noqa: E402

STRING, INT, LONG, FLOAT, DOUBLE, BOOL = 0, 1, 2, 3, 4, 5
RAW, COLS, PACKED = 0, 1, 2
MODE_NAME = {RAW: "raw", COLS: "columns", PACKED: "packed"}


def width(t):
    return 8 if t in (LONG, DOUBLE) else (1 if t == BOOL else 4)


def key_of(mode, kinds, types):
    """the words of shj_emit_key for a select list in one layout (the packed layout as
    include/siddhi_hip.h states it: 8-byte values at even words, a bool in one word,
    rows padded to 16 bytes)"""
    no = len(kinds)
    woff, colw, pos = [0] * 8, [0] * 8, 2
    for o, t in enumerate(types):
        wd = 2 if width(t) == 8 else 1
        pos = (pos + wd - 1) // wd * wd
        if mode == PACKED:
            woff[o] = pos
        if mode != RAW:
            colw[o] = width(t)
        pos += wd
    rw = (pos + 3) // 4 * 4 if mode == PACKED else 0
    pad = lambda v: list(v) + [0] * (8 - len(v))
    return [mode, no, rw] + pad(kinds) + pad(types) + woff + colw


def forms(which):
    out = []
    if "c2" in which:
        out.append(("c2", key_of(PACKED, [1, 0, 1, 1], [STRING, FLOAT, FLOAT, LONG])))
    if "c3" in which:
        out.append(("c3", key_of(RAW, [0, 0, 1], [FLOAT, FLOAT, FLOAT])))
    if "c2agg" in which:
        out.append(("c2agg", key_of(PACKED, [1, 0, 1, 1, 0, 0], [STRING, FLOAT, FLOAT, LONG, DOUBLE, DOUBLE])))
    if "synthetic" in which:
        # every width of all-4-byte and all-8-byte lists, sources alternating
        for no in range(1, 9):
            for t, tn in ((FLOAT, "f32"), (LONG, "i64")):
                for mode in (RAW, PACKED, COLS):
                    out.append((f"{no}x{tn}/{MODE_NAME[mode]}", key_of(mode, [o & 1 for o in range(no)], [t] * no)))
    if "c2raw" in which:
        for mode in (RAW, COLS):
            out.append((f"c2/{MODE_NAME[mode]}", key_of(mode, [1, 0, 1, 1], [STRING, FLOAT, FLOAT, LONG])))
    if "cases" in which:
        import emit_cases as ec
        for name, values in ec.CASES.items():
            if len(values) > 8:
                continue
            kinds = [1 if (s == 2 or a == "sym") else 0 for s, a in values]
            types = ec.types_of(values)
            for mode in (RAW, PACKED, COLS):
                out.append((f"{name}/{MODE_NAME[mode]}", key_of(mode, kinds, types)))
    return out


def source(lib, key):
    buf = C.create_string_buffer(1 << 22)
    err = C.create_string_buffer(1 << 16)
    k = (C.c_int32 * len(key))(*key)
    rc = lib.shx_emit_compile_key(k, buf, 1 << 22, err, 1 << 16)
    assert rc == abi.SH_OK, err.value.decode()[-3000:]
    return buf.value.decode()


def hipcc_form(src):
    """the hipRTC prelude's typedefs come from the HIP headers instead"""
    body = re.sub(r"^typedef __hip_internal::.*$|^typedef decltype\(sizeof\(0\)\) size_t;$|^#define INT(32|64)_MIN .*$",
                  "", src, flags=re.M)
    return "#include <hip/hip_runtime.h>\n#include <stdint.h>\n" + body


def resources(src, ru, tmp, tag):
    if ru:
        src = re.sub(r"^#define BKS_RU \d+$", f"#define BKS_RU {ru}", src, flags=re.M)
    path = os.path.join(tmp, re.sub(r"\W", "_", tag) + f"_{ru}.hip")
    with open(path, "w") as f:
        f.write(hipcc_form(src))
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-fno-gpu-flush-denormals-to-zero", "-fhip-fp32-correctly-rounded-divide-sqrt",
                        "--cuda-device-only", "-c", path, "-o", path + ".o",
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    if r.returncode:
        return {"error": r.stderr[-2000:]}
    res = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*(.*?): (\S+)", line)
        if m:
            res[m.group(1).strip()] = m.group(2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ru", default="0")
    ap.add_argument("--forms", default="c2,c3,c2agg")
    ap.add_argument("--keep", default=None, help="directory that keeps the generated sources")
    a = ap.parse_args()
    lib = abi.bind_product(C.CDLL(build.build()))
    rus = [int(x) for x in a.ru.split(",")]
    tmp = a.keep or tempfile.mkdtemp(prefix="emit_spec_")
    os.makedirs(tmp, exist_ok=True)
    jobs = []
    for tag, key in forms(a.forms.split(",")):
        src = source(lib, key)
        chosen = int(re.search(r"^#define BKS_RU (\d+)$", src, flags=re.M).group(1))
        occ = int(re.search(r"^#define BKS_OCC (\d+)$", src, flags=re.M).group(1))
        for ru in rus:
            jobs.append((tag, src, ru or chosen, occ, chosen))
    with ThreadPoolExecutor(8) as ex:
        outs = list(ex.map(lambda j: resources(j[1], j[2], tmp, j[0]), jobs))
    bad = 0
    for (tag, _, ru, occ, chosen), res in zip(jobs, outs):
        if "error" in res:
            print(f"{tag:34s} ru {ru}: COMPILE ERROR\n{res['error']}")
            bad += 1
            continue
        fits = (res.get("VGPRs Spill") == "0" and res.get("ScratchSize [bytes/lane]") == "0" and
                int(res.get("Occupancy [waves/SIMD]", "0")) >= occ)
        print(f"{tag:34s} occ {occ} ru {ru}{'*' if ru == chosen else ' '} VGPRs {res.get('VGPRs'):>4s} "
              f"spill {res.get('VGPRs Spill'):>3s} SGPRs {res.get('TotalSGPRs'):>4s} spill {res.get('SGPRs Spill'):>3s} "
              f"scratch {res.get('ScratchSize [bytes/lane]'):>4s} waves/SIMD {res.get('Occupancy [waves/SIMD]')} "
              f"{'fits' if fits else 'NO'}")
        bad += 0 if (fits or ru != chosen) else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
