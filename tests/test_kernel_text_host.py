"""Host-only checks of tools/kernel_text.py (the per-function text comparison of two device
assemblies) on two small synthetic assembly texts. No compiler, no GPU."""
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_text_mod", os.path.join(ROOT, "tools", "kernel_text.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _function(name, body, vgpr, lds, kernarg=24, end=0):
    return f"""\t.text
\t.protected\t{name}              ; -- Begin function {name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                 ; @{name}
{body}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_kernarg_size {kernarg}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{end}:
\t.size\t{name}, .Lfunc_end{end}-{name}
                                        ; -- End function
\t.set {name}.num_vgpr, {vgpr}
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
; codeLenInByte = 64
; TotalNumSgprs: 18
; NumVgprs: {vgpr}
; NumAgprs: 4
; ScratchSize: 8
; LDSByteSize: {lds} bytes/workgroup (compile time only)
; Occupancy: 7
"""


BODY_A = """; %bb.0:
\ts_load_dword s2, s[0:1], 0x10
\ts_waitcnt lgkmcnt(0)
\ts_cmp_eq_u32 s2, 0
\ts_cbranch_scc1 .LBB0_2
; %bb.1:                                ; the loop body
\tv_add_u32_e32 v1, s2, v0

\tv_mul_f32_e32 v2, v1, v1
.LBB0_2:
\ts_endpgm"""
# the same code: another label name, another comment, another blank line
BODY_A_RELABELLED = """; %bb.0:
\ts_load_dword s2, s[0:1], 0x10
\ts_waitcnt lgkmcnt(0)
\ts_cmp_eq_u32 s2, 0

\ts_cbranch_scc1 .LBB7_19
; %bb.1:                                ; a comment that changed
\tv_add_u32_e32 v1, s2, v0      ; and a new one
\tv_mul_f32_e32 v2, v1, v1
.LBB7_19:
\ts_endpgm"""
# the add and the multiply swapped
BODY_A_SWAPPED = BODY_A.replace("\tv_add_u32_e32 v1, s2, v0\n\n\tv_mul_f32_e32 v2, v1, v1",
                                "\tv_mul_f32_e32 v2, v1, v1\n\tv_add_u32_e32 v1, s2, v0")
BODY_B = "\tv_mov_b32_e32 v0, 0\n\ts_endpgm"


def test_relabelled_and_recommented_code_is_identical():
    kt = _tool()
    a = kt.parse(_function("k_one", BODY_A, 3, 1024) + _function("k_two", BODY_B, 1, 0, end=1))
    b = kt.parse(_function("k_two", BODY_B, 1, 0, end=0) + _function("k_one", BODY_A_RELABELLED, 3, 1024, end=1))
    rows, bad = kt.compare(a, b)
    assert bad == 0
    assert {r[0]: r[5] for r in rows} == {"k_one": "IDENTICAL", "k_two": "IDENTICAL"}
    assert a["k_one"].text == ["s_load_dword s2, s[0:1], 0x10", "s_waitcnt lgkmcnt(0)", "s_cmp_eq_u32 s2, 0",
                               "s_cbranch_scc1 .L", "v_add_u32_e32 v1, s2, v0", "v_mul_f32_e32 v2, v1, v1", "s_endpgm"]


def test_one_swapped_pair_differs_by_two_lines():
    kt = _tool()
    assert BODY_A_SWAPPED != BODY_A
    a = kt.parse(_function("k_one", BODY_A, 3, 1024))
    b = kt.parse(_function("k_one", BODY_A_SWAPPED, 3, 1024))
    rows, bad = kt.compare(a, b)
    assert bad == 1
    (name, na, nb, _, _, verdict), = rows
    assert (name, na, nb, verdict) == ("k_one", 7, 7, "DIFFER (2 lines)")


def test_missing_function_is_reported_and_union_finds_it():
    kt = _tool()
    one, two = _function("k_one", BODY_A, 3, 1024), _function("k_two", BODY_B, 1, 0, end=1)
    a = kt.parse(one + two)
    rows, bad = kt.compare(a, kt.parse(one))
    assert bad == 1 and {r[0]: r[5] for r in rows} == {"k_one": "IDENTICAL", "k_two": "MISSING in B"}
    # the two functions in two files taken as one side; a function only B has is listed, not an error
    extra = _function("k_three", BODY_B, 1, 0)
    rows, bad = kt.compare(a, kt.parse_union([_function("k_two", BODY_B, 1, 0), one, extra]))
    assert bad == 0
    assert {r[0]: r[5] for r in rows} == {"k_one": "IDENTICAL", "k_two": "IDENTICAL", "k_three": "only in B"}
    out = io.StringIO()
    kt.report(rows, out)
    assert "k_three | - 2 |" in out.getvalue()


def test_resource_fields_are_parsed_and_compared():
    kt = _tool()
    a = kt.parse(_function("k_one", BODY_A, 3, 1024, kernarg=24))
    assert a["k_one"].res == {"VGPR": 3, "AGPR": 4, "SGPR": 18, "LDS": 1024, "scratch": 8, "occupancy": 7,
                              "kernarg": 24}
    # the same text with other resources (more LDS, a longer argument block) is not IDENTICAL
    for other in (_function("k_one", BODY_A, 3, 2048), _function("k_one", BODY_A, 3, 1024, kernarg=32)):
        rows, bad = kt.compare(a, kt.parse(other))
        assert bad == 1 and rows[0][5] == "RESOURCES DIFFER"


def test_command_line_exit_status(tmp_path):
    kt = _tool()
    pa, pb, pc = (tmp_path / n for n in ("a.s", "b.s", "c.s"))
    pa.write_text(_function("k_one", BODY_A, 3, 1024) + _function("k_two", BODY_B, 1, 0, end=1))
    pb.write_text(_function("k_one", BODY_A_RELABELLED, 3, 1024))
    pc.write_text(_function("k_two", BODY_B, 1, 0))
    assert kt.main([str(pa), "--union", str(pb), str(pc)]) == 0
    assert kt.main([str(pa), str(pb)]) == 1  # k_two is missing
    pc.write_text(_function("k_one", BODY_A_SWAPPED, 3, 1024) + _function("k_two", BODY_B, 1, 0, end=1))
    assert kt.main([str(pa), str(pc)]) == 1  # k_one differs
