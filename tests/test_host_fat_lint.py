"""Host: build.lint_fat_dma, the build's check on the disassembly of csrc/gemm_dr_fat.hip -- a ds_read_b128 behind a 16-byte LDS-DMA
load needs an s_waitcnt vmcnt(0) in between, and the k loop carries no spill and no register move."""
from gdmcf_amd.build import lint_fat_dma

HEAD = "_ZN12_GLOBAL__N_113dr_fat_kernelILi11ELi2ELi1EEEvNS_6DrArgsE: ; @kernel\n"
LOOP = """.LBB0_1:
  s_waitcnt vmcnt(0) lgkmcnt(10)
  ds_read_b128 v[36:39], v253
  v_mfma_f32_16x16x4_f32 a[0:3], v0, v36, a[0:3]
  s_mov_b32 m0, s40
  buffer_load_dwordx4 v112, s[72:75], s3 offen lds
  s_cbranch_scc1 .LBB0_1
.LBB0_2:
  s_waitcnt vmcnt(0)
  ds_read_b128 v[36:39], v253
  s_endpgm
"""


def test_clean_kernel_passes():
    assert lint_fat_dma(HEAD + LOOP) == []


def test_read_behind_a_dma_load_without_the_wait_fails():
    bad = lint_fat_dma(HEAD + LOOP.replace(".LBB0_2:\n  s_waitcnt vmcnt(0)\n", ".LBB0_2:\n  s_waitcnt lgkmcnt(0)\n"))
    assert len(bad) == 1 and "no s_waitcnt vmcnt(0)" in bad[0]
    bad = lint_fat_dma(HEAD + LOOP.replace("vmcnt(0) lgkmcnt(10)", "vmcnt(1) lgkmcnt(10)").replace(".LBB0_2:\n  s_waitcnt vmcnt(0)\n", ".LBB0_2:\n"))
    assert len(bad) == 1 and "no s_waitcnt vmcnt(0)" in bad[0]


def test_moves_in_the_k_loop_fail():
    for ins in ("v_accvgpr_read_b32 v88, a140", "v_mov_b64_e32 v[28:29], v[124:125]", "scratch_store_dwordx4 off, v[0:3], off"):
        bad = lint_fat_dma(HEAD + LOOP.replace("  s_mov_b32 m0, s40\n", f"  {ins}\n  s_mov_b32 m0, s40\n"))
        assert len(bad) == 1 and "in the k loop" in bad[0], ins


def test_a_kernel_without_dma_loads_is_reported():
    assert lint_fat_dma(HEAD + LOOP.replace(" lds", "")) != []
    assert lint_fat_dma(HEAD.replace("dr_fat_kernel", "other_kernel") + LOOP) != []
