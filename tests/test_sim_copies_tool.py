"""tools/sim_copies.py on a small hand-written listing: kernel selection, the
loop-header blocks (from the compiler's "Loop Header" comments), runs of four
or more copies (waits and s_nop do not end a run), the totals and the
resource figures of the kernel's trailer and metadata."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """\t.text
other_kernel:                           ; @other_kernel
\tv_mov_b32_e32 v0, 0
\ts_endpgm
.Lfunc_end0:
; NumVgprs: 1
; ScratchSize: 0
my_k_sim:                               ; @my_k_sim
\t.loc\t1 10 0
\ts_load_dword s4, s[0:1], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB1_1:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB1_2 Depth 2
\t.loc\t1 20 3
\tv_mov_b32_e32 v1, v2
\tv_mov_b32_e32 v3, v4
\ts_nop 0
\ts_mov_b32 s5, s6
\ts_mov_b64 s[8:9], s[10:11]
\tv_add_u32_e32 v5, v1, v3
.LBB1_2:                                ;   Parent Loop BB1_1 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
\t.loc\t1 30 5
\tv_mov_b32_e32 v6, v5
\ts_and_saveexec_b64 s[12:13], vcc
\tv_cmp_eq_u32_e32 vcc, 0, v6
\ts_cbranch_vccnz .LBB1_2
; %bb.3:
\ts_add_i32 s5, s5, 1
\ts_cmp_lt_u32 s5, s4
\ts_cbranch_scc1 .LBB1_1
\ts_endpgm
.Lfunc_end1:
; NumVgprs: 7
; ScratchSize: 16
\t.section\t.AMDGPU.csdata
amdhsa.kernels:
  - .agpr_count:     0
    .name:           other_kernel
    .sgpr_spill_count: 9
    .symbol:         other_kernel.kd
    .vgpr_spill_count: 9
  - .agpr_count:     0
    .name:           my_k_sim
    .sgpr_spill_count: 3
    .symbol:         my_k_sim.kd
    .vgpr_spill_count: 2
"""


def load_tool():
    spec = importlib.util.spec_from_file_location("sim_copies", os.path.join(ROOT, "tools", "sim_copies.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_listing(tmp_path):
    tool = load_tool()
    path = tmp_path / "k.s"
    path.write_text(LISTING)
    ks = tool.kernels(str(path), "k_sim")
    assert list(ks) == ["my_k_sim"]
    tot, headers, per_block, note, runs = tool.analyse(*ks["my_k_sim"])
    assert headers == {".LBB1_1", ".LBB1_2"}
    assert (per_block[".LBB1_1"]["v"], per_block[".LBB1_1"]["s"], per_block[".LBB1_1"]["line"]) == (2, 2, 20)
    assert (per_block[".LBB1_2"]["v"], per_block[".LBB1_2"]["s"], per_block[".LBB1_2"]["line"]) == (1, 0, 30)
    assert [(r["block"], r["v"], r["s"]) for r in runs] == [(".LBB1_1", 2, 2)]  # s_nop inside the run
    assert tot["instructions"] == 16 and tot["v_mov"] == 3 and tot["s_mov"] == 2
    assert tot["valu"] == 5 and tot["salu"] == 5 and tot["branches"] == 2 and tot["exec_regions"] == 1
    assert tot["vgprs"] == 7 and tot["scratch"] == 16
    assert tool.spills_from_metadata(str(path), "my_k_sim") == (3, 2)
    assert tool.spills_from_metadata(str(path), "other_kernel") == (9, 9)
