"""What the compiler made of the waits of k_lbs_bwd16 and of the fc2-adjoint GEMM's prologue, read from the device assembly of the
CURRENT sources (hipcc cross-compiles gfx950 without a GPU): build.waitcnt_rows / build.asm_load_hazards.  DESIGN.md section 8
has the story; the numbers that go with it are checked on the GPU by tests/test_gpu_bwd16_waits.py."""
import importlib
import re
import subprocess

import pytest

from conftest import PKG_NAME


def _build():
    return importlib.import_module(f'{PKG_NAME}.build')


@pytest.fixture(scope='module')
def asm():
    """device assembly of the two sources, compiled once"""
    import os
    import tempfile
    b = _build()
    out = {}
    with tempfile.TemporaryDirectory(prefix='jrr_asm_') as tmp:
        jobs = {src: subprocess.Popen([b._hipcc()] + b.FLAGS + ['--cuda-device-only', '-S', os.path.join(b.CSRC, src), '-o',
                                                               os.path.join(tmp, src + '.s')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                for src in ('lbs_bwd.hip', 'gemm.hip')}
        for src, p in jobs.items():
            _, err = p.communicate()
            assert p.returncode == 0, err[-2000:]
            with open(os.path.join(tmp, src + '.s')) as f:
                out[src] = f.read()
    return out


# the shape of what the parent of this change compiled the tile loop to: a full drain behind the prefetch it has just issued, another
# in front of the first product that reads the previous prefetch, a flush block (no matrix instruction) that may drain, and a counted
# barrier wait of ours
SAMPLE = """
_ZN3jrr6k_demoILi0EEEvPKf:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dword v9, v[0:1], off
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
\t;;#ASMSTART
\ts_waitcnt vmcnt(12) lgkmcnt(0)
\ts_barrier
\t;;#ASMEND
\tglobal_load_dwordx4 v[10:13], v[2:3], off nt
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tv_mfma_f32_16x16x4_f32 v[20:23], v8, v9, v[20:23]
\ts_cbranch_scc1 .LBB0_3
; %bb.2:                                ;   in Loop: Header=BB0_1 Depth=1
\tglobal_load_dword v30, v[4:5], off sc1
\ts_waitcnt vmcnt(0)
\tglobal_store_dword v[4:5], v30, off sc1
.LBB0_3:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_waitcnt vmcnt(0)
\tv_mul_f32_e32 v40, v14, v20
\tv_mfma_f32_16x16x4_f32 v[24:27], v8, v40, v[24:27]
\ts_waitcnt vmcnt(3)
\tv_mfma_f32_16x16x4_f32 v[24:27], v8, v41, v[24:27]
\ts_cbranch_vccnz .LBB0_5
; %bb.4:                                ;   in Loop: Header=BB0_1 Depth=1
\ts_branch .LBB0_1
.LBB0_5:
\ts_waitcnt vmcnt(0)
\ts_endpgm
.Lfunc_end0:
"""


def test_the_helper_reports_full_drains_in_matrix_blocks_and_leaves_ours_out():
    rows = _build().waitcnt_rows(asm={'demo': SAMPLE})
    assert {r['name'] for r in rows} == {'jrr::k_demo<0>'}
    in_loop = [r for r in rows if r['loop'] == '.LBB0_1']
    # ours (vmcnt(12) between ;;#ASMSTART and ;;#ASMEND) is not listed; the flush block's drain is, with no matrix instruction beside it
    assert [(r['block'], r['vmcnt'], r['mfma'] > 0) for r in in_loop] == [('.LBB0_1', 0, True), ('.LBB0_1+1', 0, False), ('.LBB0_3', 0, True),
                                                                         ('.LBB0_3', 3, True)]
    assert [r['loads'] for r in in_loop] == [1, 1, 0, 0]
    outside = [r for r in rows if r['loop'] is None]
    assert [r['vmcnt'] for r in outside] == [None, 0]           # the prologue's lgkmcnt wait and the drain behind the loop


HAZARD = """
_ZN3jrr6k_demoILi1EEEvPKf:
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
\t;;#ASMSTART
\tglobal_load_dwordx4 v[10:13], v2, s[0:1] nt
\t;;#ASMEND
\tv_mov_b32_e32 v50, v11
\t;;#ASMSTART
\ts_waitcnt vmcnt(12) ; landed v[10:13]
\t;;#ASMEND
\tv_mul_f32_e32 v40, v10, v20
\ts_branch .LBB1_1
.Lfunc_end1:
"""


def test_the_hazard_walk_finds_a_copy_between_an_asm_load_and_its_wait():
    b = _build()
    found = b.asm_load_hazards({'demo': HAZARD})
    assert len(found) == 1 and 'v_mov_b32_e32 v50, v11' in found[0], found
    assert b.asm_load_hazards({'demo': HAZARD.replace('\tv_mov_b32_e32 v50, v11\n', '')}) == []
    unwaited = b.asm_load_hazards({'demo': HAZARD.replace(' ; landed v[10:13]', '')})
    assert any('no `landed` wait' in h for h in unwaited), unwaited


def test_k_lbs_bwd16_tile_loop_has_no_full_drain_beside_matrix_work(asm):
    """every instantiation (DV 0 / 1 / 2, 8 / 12 joint slots, WIDE, LIST): no basic block of the tile loop that holds a matrix
    instruction holds a compiler-emitted vmcnt(0).  (The flush blocks hold none and may drain.)  On the parent of this change the
    same helper lists three per tile pair in the headline instantiation -- DESIGN.md section 8 quotes them."""
    rows = [r for r in _build().waitcnt_rows(asm={'lbs_bwd.hip': asm['lbs_bwd.hip']}) if 'k_lbs_bwd16<' in r['name']]
    names = {r['name'] for r in rows}
    assert len(names) == 16, sorted(names)                      # 4 x (8, 12) x WIDE, DV = 0 also LIST
    bad = [(r['name'], r['block'], r['text']) for r in rows if r['loop'] is not None and r['mfma'] > 0 and r['vmcnt'] == 0]
    assert not bad, bad
    # the loop is there and was recognised: each instantiation has compiler waits (LDS) inside a loop beside matrix instructions
    for n in names:
        assert any(r['name'] == n and r['loop'] is not None and r['mfma'] > 0 for r in rows), n


def test_k_lbs_bwd16_asm_loads_reach_their_wait_untouched(asm):
    """the prefetch is issued from inline asm, invisible to the compiler: nothing may name its registers before the hand-written wait"""
    text = asm['lbs_bwd.hip']
    assert len(re.findall(r'; landed v\[', text)) >= 16 * 4      # prologue, two tiles, the wait behind the loop -- per instantiation
    assert _build().asm_load_hazards({'lbs_bwd.hip': text}) == []


def test_fc2_adjoint_gemm_prologue_loads_its_dot_partials_together(asm):
    """BTR == 2: the dz prologue sums nzpart (16) dot partials.  As a load-and-add loop it compiled to one load and one full drain per
    partial; now a block that drains has issued (at least) sixteen loads"""
    rows = [r for r in _build().waitcnt_rows(asm={'gemm.hip': asm['gemm.hip']}) if re.search(r'k_disc_gemm<\d+, \d+, \d+, \d+, 2, \d+>', r['name'])]
    assert len({r['name'] for r in rows}) == 3
    per_partial = [(r['name'], r['block'], r['loads']) for r in rows if r['loop'] is not None and r['mfma'] == 0 and r['vmcnt'] == 0 and 0 < r['loads'] < 16]
    assert not per_partial, per_partial
    for n in {r['name'] for r in rows}:
        assert any(r['name'] == n and r['mfma'] == 0 and r['vmcnt'] == 0 and r['loads'] >= 16 for r in rows), n
