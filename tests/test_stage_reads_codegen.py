"""Where the matrix kernels' LDS operand reads and epilogue loads stand in the device assembly of the CURRENT sources (hipcc cross-compiles
gfx950 without a GPU): build.memory_rows / build.lds_wait_rows / build.overlapping_lds_reads.  DESIGN.md section 8 has the story
(operand reads ahead of the chunk / stage barrier, epilogue loads in one batch, global instead of flat stores); what the kernels compute
is checked on the GPU by tests/test_gpu_stage_reads.py."""
import importlib
import os
import re
import subprocess
import tempfile

import pytest

from conftest import PKG_NAME


def _build():
    return importlib.import_module(f'{PKG_NAME}.build')


@pytest.fixture(scope='module')
def asm():
    """device assembly of the three sources, compiled once"""
    b = _build()
    out = {}
    with tempfile.TemporaryDirectory(prefix='jrr_asm_') as tmp:
        jobs = {src: subprocess.Popen([b._hipcc()] + b.FLAGS + ['--cuda-device-only', '-S', os.path.join(b.CSRC, src), '-o',
                                                               os.path.join(tmp, src + '.s')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                for src in ('lbs_fwd.hip', 'gemm.hip', 'chain.hip')}
        for src, p in jobs.items():
            _, err = p.communicate()
            assert p.returncode == 0, err[-2000:]
            with open(os.path.join(tmp, src + '.s')) as f:
                out[src] = f.read()
    return out


MFMA = '\tv_mfma_f32_32x32x2_f32 v[20:35], v{a}, v{b}, v[20:35]\n'
# k_demo<2>: what the parent of this change compiled a chunk loop to -- barrier (ours), copies, the first operand reads and a full LDS wait
# directly behind them; then reads one group ahead, as the source intends; then a narrowed read packed into the read before it with a
# wait between the two; a flat and a global store.
# k_demo<3>: a software pipeline -- the reads consumed at the top of an iteration were issued two matrix instructions before its end (the
# reads in front of the loop belong to the first iteration only).
SAMPLE = ("""
_ZN3jrr6k_demoILi2EEEvPKf:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB2_1:                                ; =>This Inner Loop Header: Depth=1
\t;;#ASMSTART
\ts_waitcnt vmcnt(6) lgkmcnt(0)
\ts_barrier
\t;;#ASMEND
\tglobal_load_lds_dwordx4 v[2:3], off
\tds_read_b128 v[10:13], v4
\tds_read_b128 v[14:17], v4 offset:512
\ts_waitcnt lgkmcnt(0)
""" + MFMA.format(a=10, b=14) + """\tds_read_b128 v[40:43], v4 offset:1024
\tds_read_b128 v[44:47], v4 offset:1536
""" + MFMA.format(a=11, b=15) + MFMA.format(a=12, b=16) + MFMA.format(a=13, b=17) + """\ts_waitcnt lgkmcnt(0)
""" + MFMA.format(a=40, b=44) + """\tds_read_b128 v[50:53], v4 offset:2048
\ts_waitcnt lgkmcnt(0)
\tds_read_b128 v[52:55], v4 offset:2064
\ts_waitcnt lgkmcnt(0)
""" + MFMA.format(a=50, b=54) + """\tflat_store_dwordx4 v[6:7], v[20:23]
\tglobal_store_dwordx4 v8, v[24:27], s[0:1]
\ts_cbranch_scc1 .LBB2_1
; %bb.2:
\ts_endpgm
.Lfunc_end2:
_ZN3jrr6k_demoILi3EEEvPKf:
; %bb.0:
\tds_read_b128 v[10:13], v4
.LBB3_1:                                ; =>This Inner Loop Header: Depth=1
\ts_waitcnt lgkmcnt(0)
""" + MFMA.format(a=10, b=11) + """\tds_read_b128 v[10:13], v4 offset:512
""" + MFMA.format(a=12, b=13) + MFMA.format(a=12, b=13) + """\ts_cbranch_scc1 .LBB3_1
; %bb.2:
\ts_endpgm
.Lfunc_end3:
""")


def test_the_helpers_see_a_zero_distance_read_a_flat_store_and_an_overlap():
    b = _build()
    rows = b.lds_wait_rows(asm={'demo': SAMPLE})
    two = [r for r in rows if r['name'] == 'jrr::k_demo<2>']
    # ours (between ;;#ASMSTART and ;;#ASMEND) is not listed, nor is the wait for the kernel arguments in front of the loop
    assert [(r['reads'], r['mfma'], r['mfma_youngest'], r['lgkmcnt']) for r in two] == [(2, 0, 0, 0), (2, 3, 3, 0), (1, 0, 0, 0), (1, 0, 0, 0)]
    assert all(r['loop'] == '.LBB2_1' and r['ops'] == ['ds_read_b128'] * r['reads'] for r in two)
    three = [r for r in rows if r['name'] == 'jrr::k_demo<3>']
    assert [(r['reads'], r['mfma']) for r in three] == [(1, 2)]          # the steady state, not the first iteration's (1, 0)
    mem = {r['name']: r for r in b.memory_rows(asm={'demo': SAMPLE})}
    m = mem['jrr::k_demo<2>']
    assert (m['flat'], m['glob'], m['lds_dma'], m['lds']) == (1, 1, 1, 6) and m['flat_text'] == ['flat_store_dwordx4 v[6:7], v[20:23]']
    assert mem['jrr::k_demo<3>']['flat'] == 0
    found = b.overlapping_lds_reads({'demo': SAMPLE})
    assert len(found) == 1 and 'v[50:53]' in found[0] and 'v[52:55]' in found[0], found
    # a reader of the first read's registers between the two makes the pair legitimate
    used = SAMPLE.replace('\tds_read_b128 v[52:55]', MFMA.format(a=50, b=51) + '\tds_read_b128 v[52:55]')
    assert b.overlapping_lds_reads({'demo': used}) == []


INNER_ITERATION = r'jrr::(k_lbs_fwd<|k_blend_adjoint<|k_disc_gemm<|k_prep_fwd_dconv$|k_dconv_bwd_reduce$)'


def test_no_flat_memory_instruction_in_the_kernels_of_the_inner_iteration(asm):
    """row bases pinned to SGPR pairs (urow, quad_ptr, pm_store) carry the global address space again: a flat store counts in lgkmcnt too,
    so every LDS wait behind it waited for the store's address phase"""
    rows = [r for r in _build().memory_rows(asm=asm) if re.match(INNER_ITERATION, r['name'])]
    names = {r['name'] for r in rows}
    assert sum('k_lbs_fwd<' in n for n in names) == 28 and sum('k_disc_gemm<' in n for n in names) == 13, sorted(names)
    assert sum('k_blend_adjoint<' in n for n in names) == 2 and {'jrr::k_prep_fwd_dconv', 'jrr::k_dconv_bwd_reduce'} <= names
    bad = [(r['name'], r['flat_text'][:2]) for r in rows if r['flat']]
    assert not bad, bad
    for r in rows:
        assert r['glob'] > 0 and r['lds'] > 0, r['name']


def _quad_waits(rows, pattern):
    """compiler waits inside a loop that wait for at least one 16- or 8-byte operand read (the quad operands of the chunk / blend loops; the
    skinning and regressor stages of k_lbs_fwd read single K steps: ds_read_b32 / ds_read2st64_b32)"""
    return [r for r in rows if pattern in r['name'] and any(o.endswith('b128') or o.endswith('b64') for o in r['ops'])]


def test_chunk_loop_of_the_disc_gemm_waits_for_no_read_it_has_just_issued(asm):
    """k_disc_gemm, every tile shape and epilogue: every compiler lgkmcnt wait of the chunk loop has matrix instructions between the
    reads it waits for and itself -- a quad pair's worth less one inside a chunk and at the chunk boundary alike (WM = 1: 3, WM = 2: 7,
    WM = 3: 11).  On the parent of this change the helper lists one zero-distance wait per chunk in every instantiation."""
    rows = _build().lds_wait_rows(asm={'gemm.hip': asm['gemm.hip']})
    waits = _quad_waits(rows, 'jrr::k_disc_gemm<')
    assert len({r['name'] for r in waits}) == 13, sorted({r['name'] for r in waits})
    for r in waits:
        wm = int(re.match(r'jrr::k_disc_gemm<(\d+),', r['name']).group(1))
        assert r['mfma'] == 4 * wm - 1, (r['name'], r['loop'], r['text'], r['reads'], r['mfma'])


def test_the_loops_left_as_they_were_are_listed_by_name(asm):
    """The same boundary was built for k_blend_adjoint (chunks) and for the blend stages of k_lbs_fwd and measured SLOWER on the GPU
    (the barrier moves ahead of the trailing matrix instructions and asks for the next copies that much earlier),
    so these loops keep their zero-distance read per chunk / stage -- the exceptions, by name and with their counts, so that a change
    of either shows up here:
      k_blend_adjoint<false>, <true>            one per chunk
      k_lbs_fwd<...>, all 28 instantiations     the first read of every blend stage but those the compiler's own schedule covers (9 or
                                                10 per tile), and the skinning / regressor stages, whose reads depend on a matrix
                                                result (single K steps, not counted here)
    and group 3 of the last blend chunk of k_lbs_fwd keeps the 16-byte reads the compiler narrows into overlapping registers (8-byte
    reads were measured slower as well): build.overlapping_lds_reads lists them, in lbs_fwd.hip only."""
    b = _build()
    rows = b.lds_wait_rows(asm={k: asm[k] for k in ('gemm.hip', 'lbs_fwd.hip')})
    adj = _quad_waits(rows, 'jrr::k_blend_adjoint<')
    for n in ('jrr::k_blend_adjoint<false>', 'jrr::k_blend_adjoint<true>'):
        assert sorted(r['mfma'] for r in adj if r['name'] == n) == [0, 27], n
    fwd = _quad_waits(rows, 'jrr::k_lbs_fwd<')
    names = {r['name'] for r in fwd}
    assert len(names) == 28, sorted(names)
    for n in names:
        zero = sum(1 for r in fwd if r['name'] == n and r['mfma'] == 0)
        assert zero in (9, 10), (n, zero)
        assert {r['mfma'] for r in fwd if r['name'] == n} <= {0, 11}, n
    assert b.overlapping_lds_reads({'gemm.hip': asm['gemm.hip']}) == []
    found = b.overlapping_lds_reads({'lbs_fwd.hip': asm['lbs_fwd.hip']})
    assert found and all('k_lbs_fwd' in f for f in found), found[:3]


def test_disc_gemm_epilogues_load_before_their_first_wait(asm):
    """bias / dot-weight / mask quads of the wave's WM x 4 output quads: all requested in front of the first vmcnt wait behind the first of
    them (they were one load and one wait per output quad)"""
    b = _build()
    fns = list(b._functions(asm['gemm.hip']))
    names = b._demangled(n for n, _ in fns)
    seen = 0
    for mangled, items in fns:
        m = re.match(r'jrr::k_disc_gemm<(\d+), \d+, \d+, (\d+), \d+, \d+>', names[mangled])
        if not m or int(m.group(2)) == 0:          # EPI_STORE loads nothing
            continue
        wm, epi = int(m.group(1)), int(m.group(2))
        ins = [p for k, p in items if k == 'ins']
        last = max(i for i, (t, _) in enumerate(ins) if t.startswith('v_mfma'))
        tail = ins[last + 1:]
        first_load = next(i for i, (t, _) in enumerate(tail) if t.startswith('global_load'))       # (behind the K-split reduction's barriers)
        first_wait = next(i for i, (t, ours) in enumerate(tail) if i > first_load and t.startswith('s_waitcnt') and 'vmcnt' in t and not ours)
        before = sum(1 for t, _ in tail[:first_wait] if t.startswith('global_load'))
        after = sum(1 for t, _ in tail[first_wait:] if t.startswith('global_load') or t.startswith('flat_load'))
        assert after == 0, (names[mangled], after)
        assert before == wm * 4 * (2 if epi == 5 else 1), (names[mangled], before)      # EPI_BIAS_RELU_DOT: bias and dot weights
        seen += 1
    assert seen == 9
