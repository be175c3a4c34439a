"""Build the gfx950 shared library (csrc/*.hip -> libjrr_hip.so) with hipcc, in-tree.

    python joint-regressor-refinement_amd/build.py [--force] [--report] [--clean]

hipcc cross-compiles for gfx950 without a GPU.  The .so is git-ignored but travels with the
repo snapshot to the GPU box.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(HERE, 'build')
LIB = os.path.join(HERE, 'libjrr_hip.so')
SOURCES = ['api.hip', 'model.hip', 'refine.hip', 'rot.hip', 'chain.hip', 'loss.hip', 'flat.hip', 'lbs_fwd.hip', 'lbs_bwd.hip', 'jreg.hip', 'gemm.hip', 'disc.hip', 'eval.hip', 'fold.hip', 'sil.hip', 'sup.hip', 'image.hip', 'report.hip', 'shade.hip', 'export.hip', 'evalrep.hip', 'evalproto.hip', 'smooth.hip', 'regrep.hip', 'views.hip', 'accel.hip', 'pve.hip', 'jfit.hip', 'jmom.hip', 'jnorm.hip', 'boot.hip', 'jprice.hip', 'depth.hip', 'bones.hip', 'pen.hip', 'place.hip', 'vis.hip']
HEADERS = ['jrr_common.h', 'kernels.h', 'lbs_tile.h', 'engine.h', 'engine_state.h','dconv.h', 'supk.h', 'chaink.h', 'proj.h', 'rot6.h', 'quat.h', 'evalk.h', 'procfit.h', 'jfitk.h', 'fixedpt.h', 'acctab.h', os.path.join('..', '..', 'include', 'jrr.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-Wall', '-Wno-unused-function']


def _hipcc() -> str:
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return 'hipcc'


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def resource_rows(sources=None):
    """Per-kernel resource usage of the CURRENT sources (compiled into a scratch directory with
    -Rpass-analysis=kernel-resource-usage; the in-tree objects are not touched): a list of dicts with the demangled kernel
    name and integer vgpr / agpr / scratch / vspill / occ / lds.  tests/test_host_logic.py fails on any spilled register."""
    import tempfile
    tmp = tempfile.mkdtemp(prefix='jrr_report_')
    jobs = [[_hipcc()] + FLAGS + ['-c', os.path.join(CSRC, src), '-o', os.path.join(tmp, src.replace('.hip', '.o')),
                                  '-Rpass-analysis=kernel-resource-usage'] for src in (sources or SOURCES)]
    with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as ex:
        outs = list(ex.map(lambda cmd: subprocess.run(cmd, capture_output=True, text=True), jobs))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    rows = []
    for p in outs:
        if p.returncode != 0:
            raise RuntimeError('hipcc failed:\n' + p.stderr[-2000:])
        rows += _parse(p.stdout + p.stderr)
    return rows


def _parse(out: str):
    import re
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            try:
                name = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip() or name
            except OSError:
                pass
            cur = {'name': name.split('(')[0]}
            rows.append(cur)
            continue
        for key, pat in (('vgpr', r'remark:\s+VGPRs: (\d+)'), ('agpr', r'AGPRs: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('occ', r'Occupancy \[waves/SIMD\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)'),
                         ('vspill', r'VGPRs Spill: (\d+)')):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return [r for r in rows if 'vgpr' in r]


def waitcnt_rows(sources=None, asm=None):
    """The s_waitcnt instructions THE COMPILER inserted, per kernel, of the CURRENT sources (device assembly compiled into a scratch
    directory; `asm`: a dict {source name: assembly text} to parse instead).  Waits written in inline asm (between ;;#ASMSTART and
    ;;#ASMEND) are ours and are left out.  One dict per wait:
        name    demangled kernel name with its template arguments (no parameter list)
        loop    label of the header of the innermost loop around the wait's basic block, None outside every loop
        depth   nesting depth of that loop (0 outside)
        block   the basic block: its label, or `label+k` for the k-th block behind a branch that has no label of its own
        text    the instruction
        vmcnt   the vmcnt it waits for, None if it has no vmcnt field (vmcnt 0 = a full drain of loads, stores and LDS-DMA)
        mfma    matrix instructions in the same basic block
        loads   global / buffer loads in the same basic block
    A kernel that prefetches into registers wants COUNTED waits (vmcnt(N), N > 0) in the blocks of its main loop that do the matrix
    work: tests/test_waitcnt_codegen.py."""
    import re
    import tempfile
    import shutil
    if asm is None:
        tmp = tempfile.mkdtemp(prefix='jrr_asm_')
        names = list(sources or SOURCES)
        jobs = [[_hipcc()] + FLAGS + ['--cuda-device-only', '-S', os.path.join(CSRC, src), '-o', os.path.join(tmp, src.replace('.hip', '.s'))]
                for src in names]
        with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as ex:
            outs = list(ex.map(lambda cmd: subprocess.run(cmd, capture_output=True, text=True), jobs))
        asm = {}
        try:
            for src, p in zip(names, outs):
                if p.returncode != 0:
                    raise RuntimeError('hipcc failed:\n' + p.stderr[-2000:])
                with open(os.path.join(tmp, src.replace('.hip', '.s'))) as f:
                    asm[src] = f.read()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    rows = []
    for text in asm.values():
        rows += _waitcnt_parse(text)
    mangled = sorted({r['name'] for r in rows})
    if mangled:
        try:
            dem = subprocess.run(['c++filt'], input='\n'.join(mangled), capture_output=True, text=True).stdout.splitlines()
        except OSError:
            dem = []
        if len(dem) == len(mangled):
            table = dict(zip(mangled, dem))
            for r in rows:
                full = table[r['name']]
                # cut the parameter list, keep the template arguments: `void jrr::k<0, 8, false>(float const*, ...)`
                depth, cut = 0, len(full)
                for i, ch in enumerate(full):
                    if ch == '<':
                        depth += 1
                    elif ch == '>':
                        depth -= 1
                    elif ch == '(' and depth == 0:
                        cut = i
                        break
                r['name'] = full[:cut].replace('void ', '', 1)
    return rows


def _waitcnt_parse(text: str):
    import re
    rows = []
    lines = text.splitlines()
    i = 0
    fn_re = re.compile(r'^(_Z\w+):')
    lab_re = re.compile(r'^(\.LBB\d+_\d+):(.*)$')
    while i < len(lines):
        m = fn_re.match(lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        i += 1
        # basic blocks of the function: a label opens one, a branch closes one
        blocks, cur = [], {'label': 'entry', 'loop': None, 'depth': 0, 'ins': []}
        last_label, sub, in_asm, hdr_depth = 'entry', 0, False, {}
        while i < len(lines) and not lines[i].startswith('.Lfunc_end'):
            ln = lines[i]
            i += 1
            lm = lab_re.match(ln)
            if lm:
                blocks.append(cur)
                label, note = lm.group(1), lm.group(2)
                loop, depth = None, 0
                h = re.search(r'Loop Header: Depth=(\d+)', note)
                if h:
                    loop, depth = label, int(h.group(1))
                    hdr_depth[label] = depth
                else:
                    h = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', note)
                    if h:
                        loop, depth = '.L' + h.group(1), int(h.group(2))
                cur = {'label': label, 'loop': loop, 'depth': depth, 'ins': []}
                last_label, sub = label, 0
                continue
            s = ln.strip()
            if s.startswith(';;#ASMSTART'):
                in_asm = True
                continue
            if s.startswith(';;#ASMEND'):
                in_asm = False
                continue
            if not s or s.startswith(';') or s.startswith('.'):
                continue
            ins = s.split(';')[0].strip()
            if not ins:
                continue
            cur['ins'].append((ins, in_asm))
            b = re.match(r's_c?branch\w*\s+(\.LBB\d+_\d+)', ins)
            if b:
                blocks.append(cur)
                sub += 1
                # the block behind a branch belongs to the loop of the block before it -- unless that branch was the loop's back edge
                loop, depth = cur['loop'], cur['depth']
                if loop is not None and b.group(1) == loop:
                    loop, depth = None, 0
                cur = {'label': f'{last_label}+{sub}', 'loop': loop, 'depth': depth, 'ins': []}
        blocks.append(cur)
        for blk in blocks:
            mfma = sum(1 for ins, _ in blk['ins'] if ins.startswith('v_mfma'))
            loads = sum(1 for ins, _ in blk['ins'] if re.match(r'(global|buffer|flat)_load', ins))
            for ins, ours in blk['ins']:
                if ours or not ins.startswith('s_waitcnt'):
                    continue
                v = re.search(r'vmcnt\((\d+)\)', ins)
                rows.append({'name': name, 'loop': blk['loop'], 'depth': blk['depth'], 'block': blk['label'], 'text': ins,
                             'vmcnt': int(v.group(1)) if v else None, 'mfma': mfma, 'loads': loads})
    return rows


def _device_asm(sources=None):
    """{source name: device assembly text} of the CURRENT sources, compiled into a scratch directory"""
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp(prefix='jrr_asm_')
    names = list(sources or SOURCES)
    jobs = [[_hipcc()] + FLAGS + ['--cuda-device-only', '-S', os.path.join(CSRC, src), '-o', os.path.join(tmp, src.replace('.hip', '.s'))]
            for src in names]
    try:
        with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as ex:
            outs = list(ex.map(lambda cmd: subprocess.run(cmd, capture_output=True, text=True), jobs))
        asm = {}
        for src, p in zip(names, outs):
            if p.returncode != 0:
                raise RuntimeError('hipcc failed:\n' + p.stderr[-2000:])
            with open(os.path.join(tmp, src.replace('.hip', '.s'))) as f:
                asm[src] = f.read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return asm


def _demangled(mangled):
    """{mangled: `jrr::k<0, 8, false>`} -- template arguments kept, parameter list and `void ` cut"""
    mangled = sorted(set(mangled))
    try:
        dem = subprocess.run(['c++filt'], input='\n'.join(mangled), capture_output=True, text=True).stdout.splitlines()
    except OSError:
        dem = []
    if len(dem) != len(mangled):
        return {m: m for m in mangled}
    table = {}
    for m, full in zip(mangled, dem):
        depth, cut = 0, len(full)
        for i, ch in enumerate(full):
            if ch == '<':
                depth += 1
            elif ch == '>':
                depth -= 1
            elif ch == '(' and depth == 0:
                cut = i
                break
        table[m] = full[:cut].replace('void ', '', 1)
    return table


def _functions(text: str):
    """(mangled name, [(kind, payload)]) per function of an assembly text, in program order: kind 'label' -> (label, rest of the line),
    kind 'ins' -> (instruction without its comment, inside ;;#ASMSTART / ;;#ASMEND?)"""
    import re
    fn_re = re.compile(r'^(_Z\w+):')
    lab_re = re.compile(r'^(\.LBB\d+_\d+):(.*)$')
    lines = text.splitlines()
    i = 0
    while i < len(lines):
        m = fn_re.match(lines[i])
        i += 1
        if not m:
            continue
        items, in_asm = [], False
        while i < len(lines) and not lines[i].startswith('.Lfunc_end'):
            ln = lines[i]
            i += 1
            lm = lab_re.match(ln)
            if lm:
                items.append(('label', (lm.group(1), lm.group(2))))
                continue
            s = ln.strip()
            if s.startswith(';;#ASMSTART'):
                in_asm = True
            elif s.startswith(';;#ASMEND'):
                in_asm = False
            elif s and not s.startswith(';') and not s.startswith('.'):
                ins = s.split(';')[0].strip()
                if ins:
                    items.append(('ins', (ins, in_asm)))
        yield m.group(1), items


def memory_rows(sources=None, asm=None):
    """The memory instructions of every kernel of the CURRENT sources by kind (`asm`: {source name: assembly text} to parse instead).
    One dict per kernel:
        name      demangled kernel name with its template arguments
        flat      flat_load / flat_store / flat_atomic: what an access through a pointer of unknown address space compiles to.  A flat
                  instruction counts in lgkmcnt AS WELL AS vmcnt -- every LDS wait behind it also waits for its address phase
        glob      global_load / global_store / global_atomic (LDS-DMA not included)
        lds_dma   global_load_lds / buffer_load ... lds
        lds       ds_read / ds_write
        flat_text the flat instructions themselves
    tests/test_stage_reads_codegen.py: no flat instruction in the kernels of the inner iteration."""
    import re
    if asm is None:
        asm = _device_asm(sources)
    rows = []
    for text in asm.values():
        for name, items in _functions(text):
            r = {'name': name, 'flat': 0, 'glob': 0, 'lds_dma': 0, 'lds': 0, 'flat_text': []}
            for kind, (ins, _) in items:
                if kind != 'ins':
                    continue
                op = ins.split()[0]
                if op.startswith('flat_'):
                    r['flat'] += 1
                    r['flat_text'].append(ins)
                elif op.startswith('global_load_lds') or (op.startswith('buffer_load') and re.search(r'\blds\b', ins)):
                    r['lds_dma'] += 1
                elif op.startswith('global_') or op.startswith('buffer_'):
                    r['glob'] += 1
                elif op.startswith('ds_'):
                    r['lds'] += 1
            rows.append(r)
    table = _demangled(r['name'] for r in rows)
    for r in rows:
        r['name'] = table[r['name']]
    return rows


def lds_wait_rows(sources=None, asm=None):
    """How far ahead of its consumer an LDS read was issued, read from the device assembly of the CURRENT sources (`asm`: {source name:
    assembly text} to parse instead): one dict per s_waitcnt THE COMPILER inserted inside a loop that has an lgkmcnt field and waits for
    at least one ds_read:
        name           demangled kernel name with its template arguments
        loop           label of the header of the innermost loop around the wait
        text           the instruction
        lgkmcnt        the count it waits for
        reads          ds_read instructions it waits for
        ops            their opcodes, oldest first (ds_read_b128: a quad operand; ds_read_b32 / ds_read2st64_b32: single K steps)
        mfma           matrix instructions issued between the OLDEST ds_read it waits for and the wait
        mfma_youngest  ... between the YOUNGEST one and the wait
    mfma == 0 is a read with prefetch distance zero: the wave requests its operand and waits for it with nothing of its own in the
    matrix pipe.  The walk follows the program text; at a loop header it continues from the state at the loop's back edge (reads
    issued at the end of an iteration and consumed at the start of the next are what a software pipeline looks like), so the rows
    describe the steady state, not the first iteration.  A wait written in inline asm empties the queue and is not listed."""
    import re
    if asm is None:
        asm = _device_asm(sources)
    rows = []
    for text in asm.values():
        for name, items in _functions(text):
            at_backedge, extents, label_at = {}, [], {}      # extents: (first, last item, header) of every backward branch
            announced = any(kind == 'label' and 'Loop Header' in payload[1] for kind, payload in items)
            for emit in (False, True):
                queue, nm, loop = [], 0, None          # queue: (opcode of a ds_read / None, matrix instructions issued before it)
                seen, fell = set(), True               # labels passed; the previous instruction falls through to the next one
                for at, (kind, payload) in enumerate(items):
                    if kind == 'label':
                        label, note = payload
                        seen.add(label)
                        label_at[label] = at
                        if 'Loop Header' in note:
                            if not emit and fell and loop == label:      # a rotated loop: its last block stands in front of the header
                                at_backedge[label] = (list(queue), nm)
                            loop = label
                            if label in at_backedge:
                                q, n0 = at_backedge[label]
                                queue = [(d, c - n0 + nm) for d, c in q]
                        else:
                            h = re.search(r'in Loop: Header=(BB\d+_\d+)', note)
                            loop = '.L' + h.group(1) if h else None
                        continue
                    ins, ours = payload
                    op = ins.split()[0]
                    fell = op != 's_branch'
                    if op.startswith('v_mfma'):
                        nm += 1
                    elif op.startswith('ds_read'):
                        queue.append((op, nm))
                    elif op.startswith('ds_') or op.startswith('s_load') or op.startswith('s_buffer_load') or op.startswith('flat_'):
                        queue.append((None, nm))
                    elif op == 's_waitcnt':
                        m = re.search(r'lgkmcnt\((\d+)\)', ins)
                        if m:
                            keep = int(m.group(1))
                            waited = queue[:len(queue) - keep] if keep else queue
                            reads = [c for d, c in waited if d]
                            ops = [d for d, c in waited if d]
                            inside = loop
                            if inside is None and not announced:      # a function whose loops the compiler's comments do not announce (an
                                # irreducible loop): the text between a label and a branch back to it
                                around = [e for e in extents if e[0] <= at <= e[1]]
                                inside = min(around, key=lambda e: e[1] - e[0])[2] if around else None
                            if emit and reads and not ours and inside is not None:
                                rows.append({'name': name, 'loop': inside, 'text': ins, 'lgkmcnt': keep, 'reads': len(reads), 'ops': ops,
                                             'mfma': nm - reads[0], 'mfma_youngest': nm - reads[-1]})
                            queue = queue[len(queue) - keep:] if keep else []
                    else:
                        b = re.match(r's_c?branch\w*\s+(\.LBB\d+_\d+)', ins)
                        if b and not emit and (b.group(1) in seen or b.group(1) == loop):      # a back edge
                            at_backedge[b.group(1)] = (list(queue), nm)
                            if b.group(1) in seen:
                                extents.append((label_at[b.group(1)], at, b.group(1)))
    table = _demangled(r['name'] for r in rows)
    for r in rows:
        r['name'] = table[r['name']]
    return rows


def overlapping_lds_reads(asm: dict):
    """Two consecutive ds_read whose destination registers overlap, with a compiler s_waitcnt and no reader of the first one's
    registers between them: the compiler narrowed a read whose upper part nobody uses and packed the next one into it, which costs a
    full LDS round trip per read.  One string per pair found in the assembly texts `asm` ({source name: text}); an empty list is what
    the kernels want."""
    import re
    out = []
    dst_re = re.compile(r'^ds_read\w*\s+v(?:\[(\d+):(\d+)\]|(\d+))')
    reg_re = re.compile(r'\bv\[(\d+):(\d+)\]|\bv(\d+)\b')
    for text in asm.values():
        for name, items in _functions(text):
            prev, waits, used = None, 0, False       # the last ds_read: (text, lo, hi); compiler waits behind it; its registers named since
            for kind, payload in items:
                if kind == 'label':
                    prev = None
                    continue
                ins, ours = payload
                m = dst_re.match(ins)
                if m:
                    lo, hi = (int(m.group(3)),) * 2 if m.group(3) is not None else (int(m.group(1)), int(m.group(2)))
                    if prev and waits and not used and lo <= prev[2] and prev[1] <= hi:
                        out.append(f'{name}: `{prev[0]}` and `{ins}` overlap, separated by a wait only')
                    prev, waits, used = (ins, lo, hi), 0, False
                elif prev:
                    if ins.startswith('s_waitcnt'):
                        waits += 0 if ours else 1
                    else:
                        for r in reg_re.finditer(ins.split(None, 1)[1] if ' ' in ins else ''):
                            a, b = (int(r.group(3)),) * 2 if r.group(3) is not None else (int(r.group(1)), int(r.group(2)))
                            if a <= prev[2] and prev[1] <= b:
                                used = True
    return out


def asm_load_hazards(asm: dict):
    """Loads issued from inline asm (csrc/jrr_common.h, quad_load) are invisible to the compiler's wait insertion: nothing but the
    hand-written `s_waitcnt vmcnt(N) ; landed v[a:b] ...` (quads_landed) stands between such a load and a reader of its
    registers.  For every `global_load_dwordx4 v[a:b]` inside ;;#ASMSTART / ;;#ASMEND of the assembly texts `asm`
    ({source name: text}, as waitcnt_rows takes them) this walks forward in program text -- round the loop once where the walk
    meets a branch back to the loop header -- to the `landed` wait that names v[a:b], and returns one string per instruction
    on the way that names one of those registers (a register copy the compiler put there to merge two paths, say).  An empty
    list is what the kernels rely on.  A load whose wait the walk does not find is reported too."""
    import re
    out = []
    reg_re = re.compile(r'\bv\[(\d+):(\d+)\]|\bv(\d+)\b')

    def regs(operand_text):
        s = set()
        for m in reg_re.finditer(operand_text):
            if m.group(3) is not None:
                s.add(int(m.group(3)))
            else:
                s.update(range(int(m.group(1)), int(m.group(2)) + 1))
        return s

    for text in asm.values():
        lines = text.splitlines()
        starts = [i for i, ln in enumerate(lines) if re.match(r'^_Z\w+:', ln)]
        for fi, f0 in enumerate(starts):
            f1 = starts[fi + 1] if fi + 1 < len(starts) else len(lines)
            name = lines[f0].split(':')[0]
            body = lines[f0:f1]
            label_at = {m.group(1): k for k, ln in enumerate(body) for m in [re.match(r'^(\.LBB\d+_\d+):', ln)] if m}
            header_of = {}
            for k, ln in enumerate(body):
                m = re.match(r'^(\.LBB\d+_\d+):(.*)$', ln)
                if m:
                    h = re.search(r'in Loop: Header=(BB\d+_\d+)', m.group(2))
                    cur = '.L' + h.group(1) if h else (m.group(1) if 'Loop Header' in m.group(2) else None)
                header_of[k] = cur if m else header_of.get(k - 1)
            in_asm = False
            for k, ln in enumerate(body):
                s = ln.strip()
                if s.startswith(';;#ASMSTART'):
                    in_asm = True
                elif s.startswith(';;#ASMEND'):
                    in_asm = False
                m = re.match(r'global_load_dwordx4\s+v\[(\d+):(\d+)\]', s) if in_asm else None
                if not m:
                    continue
                tag = f'v[{m.group(1)}:{m.group(2)}]'
                dst = set(range(int(m.group(1)), int(m.group(2)) + 1))
                pos, wrapped, found, steps = k + 1, False, False, 0
                while pos < len(body) and steps < 20000:
                    steps += 1
                    t = body[pos].strip()
                    ins = t.split(';')[0].strip()
                    if t.startswith('s_waitcnt') and 'landed' in t and tag in t:
                        found = True
                        break
                    br = re.match(r's_c?branch\w*\s+(\.LBB\d+_\d+)', ins)
                    if br and ins.startswith('s_branch') and not wrapped and header_of.get(k) is not None:
                        # the back edge: an unconditional branch up to the header, or to a block of the same loop in front of it
                        tgt = label_at.get(br.group(1), len(body))
                        if tgt < pos and (br.group(1) == header_of[k] or header_of.get(tgt) == header_of[k]):
                            pos, wrapped = tgt, True
                            continue
                    if ins and not ins.startswith('.') and not re.match(r'^\.?\w+:', ins):
                        parts = ins.split(None, 1)
                        ops = parts[1] if len(parts) > 1 else ''
                        if regs(ops) & dst:      # a reader sees stale data, a writer is overwritten when the load lands
                            out.append(f'{name}: `{ins}` touches {tag} before its wait')
                    pos += 1
                if not found:
                    out.append(f'{name}: no `landed` wait for the load into {tag}')
    return out


def _summarise(out: str) -> str:
    """Condense -Rpass-analysis=kernel-resource-usage remarks to one line per kernel."""
    import re
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r'remark: Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            try:
                name = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip() or name
            except OSError:
                pass
            cur = {'name': name.split('(')[0][:70]}
            rows.append(cur)
            continue
        for key, pat in (('vgpr', r'remark:\s+VGPRs: (\d+)'), ('agpr', r'AGPRs: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'),
                         ('occ', r'Occupancy \[waves/SIMD\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)'),
                         ('sgpr', r'remark:\s+SGPRs: (\d+)'), ('vspill', r'VGPRs Spill: (\d+)')):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = m.group(1)
        if 'warning' in line or 'error' in line:
            rows.append({'name': line})
    txt = ''
    for r in rows:
        if 'vgpr' in r:
            txt += (f"  {r['name']:<72s} vgpr={r.get('vgpr')} agpr={r.get('agpr')} sgpr={r.get('sgpr')} scratch={r.get('scratch')} "
                    f"vspill={r.get('vspill')} occ={r.get('occ')} lds={r.get('lds')}\n")
        else:
            txt += r['name'] + '\n'
    return txt


def clean(verbose: bool = True) -> list:
    """Remove every file of the object directory that is not the object of a source in SOURCES (experiment variants built by hand or by
    older tools): they would otherwise travel to the GPU box with every snapshot.  Returns the removed names."""
    keep = {s.replace('.hip', '.o') for s in SOURCES}
    gone = []
    if os.path.isdir(OBJ):
        for name in sorted(os.listdir(OBJ)):
            if name not in keep:
                os.remove(os.path.join(OBJ, name))
                gone.append(name)
    if verbose and gone:
        print(f'[jrr build] removed {len(gone)} stale objects from {OBJ}')
    return gone


def build(force: bool = False, report: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace('.hip', '.o'))
        if force or report or _stale(o, [s] + hdrs):
            cmd = [_hipcc()] + FLAGS + ['-c', s, '-o', o]
            if report:
                cmd.append('-Rpass-analysis=kernel-resource-usage')
            jobs.append((src, cmd))

    def run(job):
        src, cmd = job
        p = subprocess.run(cmd, capture_output=True, text=True)
        return src, p.returncode, p.stdout + p.stderr

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), 8)) as ex:
            for src, rc, out in ex.map(run, jobs):
                if rc != 0:
                    sys.stderr.write(out)
                elif report:
                    sys.stderr.write(_summarise(out))
                if rc != 0:
                    raise RuntimeError(f'hipcc failed on {src}')
                if verbose:
                    print(f'[jrr build] compiled {src}')
    objs = [os.path.join(OBJ, s.replace('.hip', '.o')) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        cmd = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC'] + objs + ['-o', LIB]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            raise RuntimeError('hipcc link failed')
        if verbose:
            print(f'[jrr build] linked {LIB}')
    return LIB


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--force', action='store_true')
    ap.add_argument('--report', action='store_true', help='print per-kernel VGPR/LDS/occupancy')
    ap.add_argument('--clean', action='store_true', help='remove objects that do not belong to SOURCES (stale experiment variants)')
    a = ap.parse_args()
    if a.clean:
        clean()
    build(force=a.force, report=a.report)
