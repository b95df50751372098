"""The bucketed emitter compiled per (select list, output layout), checked on the CPU:
for every list of emit_cases.CASES with at most 8 values, in each of the three
layouts, the generated source compiles for gfx950 (hipRTC needs no device), carries
the list's descriptors as constexpr tables, and has no run-time descriptor read left:
the kernel's arguments are the plan and a block of pointers, and every `O.kind[`,
`O.type[`, `OC.woff[`, `OC.colw[`, `OC.rw` of the text sits in the branch of a
`BKS_NO` conditional that the specialised build does not compile."""
import ctypes as C
import re

import pytest

import emit_cases as ec
from siddhi_amd import abi, build, compiler

MODE = {"raw": 0, "columns": 1, "packed": 2}      # SHB_OUT_*
SPEC = [n for n, v in ec.CASES.items() if len(v) <= 8]
SH_T = {ec.STRING: 0, ec.INT: 1, ec.LONG: 2, ec.FLOAT: 3, ec.DOUBLE: 4, ec.BOOL: 5}
READS = ("O.kind[", "O.type[", "O.n_out", "OC.woff[", "OC.colw[", "OC.rw", "o_kind[o] ==", "o_type[o])")


@pytest.fixture(scope="module")
def lib():
    return abi.bind_product(C.CDLL(build.build()))


def _source(lib, values, layout):
    d = compiler.compile_app(ec.app(values), ec.strings(16)).descriptor()
    h = C.c_void_p()
    assert lib.sh_compile(C.byref(d), C.byref(h)) == abi.SH_OK
    buf = C.create_string_buffer(1 << 21)
    rc = lib.shx_emit_compile(h, MODE[layout], buf, 1 << 21)
    err = lib.sh_last_error(h).decode()
    lib.sh_destroy(h)
    return rc, buf.value.decode(), err


def _compiled_text(src):
    """the lines a build with BKS_NO defined compiles, as far as BKS_NO conditionals decide
    it (no other conditional of the emitter's text holds a descriptor read)"""
    keep, stack = [], []
    for line in src.splitlines():
        t = line.strip()
        if re.match(r"#\s*if", t):
            m = re.match(r"#\s*if(n?)def\s+BKS_NO\b", t)
            stack.append(None if not m else (m.group(1) == ""))
            continue
        if t.startswith("#else") and stack:
            if stack[-1] is not None:
                stack[-1] = not stack[-1]
            continue
        if t.startswith("#endif") and stack:
            stack.pop()
            continue
        if all(s is not False for s in stack):
            keep.append(line.split("//")[0])       # (comments speak of the generic build too)
    assert not stack
    return keep


def _table(src, name):
    m = re.search(r"constexpr int32_t " + name + r"\[BKS_NO\] = \{([^}]*)\};", src)
    assert m, name
    return [int(x) for x in m.group(1).split(",")]


@pytest.mark.parametrize("layout", ec.LAYOUTS)
@pytest.mark.parametrize("name", SPEC)
def test_specialised_emitter_compiles(lib, name, layout):
    values = ec.CASES[name]
    types = ec.types_of(values)
    rc, src, err = _source(lib, values, layout)
    assert rc == abi.SH_OK, err[-3000:]
    no = len(values)
    assert f"#define BKS_NO {no}\n" in src and f"#define BKS_MODE {MODE[layout]}\n" in src
    # the tables are the list's: e2-side values and the folded partition attribute by event
    assert _table(src, "BKS_KIND") == [1 if (s == 2 or a == "sym") else 0 for s, a in values]
    assert _table(src, "BKS_TYPE") == [SH_T[t] for t in types]
    offs, row_bytes = ec.packed_layout(types)
    if layout == "packed":
        assert _table(src, "BKS_WOFF") == [o // 4 for o in offs]
        assert f"#define BKS_RW {row_bytes // 4}\n" in src
    if layout != "raw":
        assert _table(src, "BKS_COLW") == [ec.NATURAL[t] for t in types]
    # the occupancy form is the generic launcher's, and is in the kernel's name
    occ = 6 if ec.six_waves(layout, no) else 4
    assert f"#define BKS_OCC {occ}\n" in src
    m = re.search(r"#define BKS_NAME (k_bk_emit_(\d)_(\d)_(\d)_(\d))\n", src)
    assert m and (int(m.group(2)), int(m.group(3)), int(m.group(5))) == (MODE[layout], no, occ)
    assert f"#define BKS_RU {m.group(4)}\n" in src and int(m.group(4)) >= 1
    # no run-time descriptor read: not in the arguments, not in the compiled text
    body = "\n".join(_compiled_text(src[src.index("#define BKS_NO"):]))
    sig = body[body.index("BKS_NAME(shb_plan P,"):]
    sig = sig[:sig.index("{")]
    assert "shb_out" not in sig and "shb_cols" not in sig and "bks_ptrs Q" in sig
    for read in READS:
        assert read not in body, read
    assert "BKS_KIND[o]" in body and "BKS_TYPE[o]" in body


@pytest.mark.parametrize("name", [n for n in ec.CASES if n not in SPEC])
def test_longer_lists_have_no_specialised_form(lib, name):
    rc, _, err = _source(lib, ec.CASES[name], "packed")
    assert rc == abi.SH_E_UNSUPPORTED, (rc, err[-500:])
