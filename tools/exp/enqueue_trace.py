"""Enqueue trace of the library WITHOUT a GPU: the HIP runtime calls the library makes are served by a stand-in (hip_trace_stub.cpp, loaded
ahead of the library) that runs nothing and logs every enqueue -- kernel name, grid, block, LDS bytes, stream; copies and memsets with their
sizes (done on host memory); event records / waits; stream creation.  The driver below walks every shape of the fused inner loop: the
support-vertex iteration composed and as side-stream halves (the regressor's support lists are written into the workspace as the device
would have left them), its split launches, the tile-listed / all-tiles LBS chain, forward reuse after a J step, folded, silhouette, the
in-call J steps, loss history, profiling.  The "operators" section then calls every entry point that lives beside its kernels (image,
report, shade, export, eval, evalrep, regrep, smooth; the discriminator and silhouette operators on the engines built before) once at
the smallest sizes it accepts and once with an argument it refuses; the status and jrr_last_error() of the refusal are part of the
trace.  Two libraries that print the same trace enqueue the same work in the same order (the kernels'
ARGUMENTS are not compared: that is what the bit-for-bit comparison of results on a GPU is for).

    python tools/exp/enqueue_trace.py <libA.so> <libB.so> [outdir]     compares the two under the default environment and each loop knob
    python tools/exp/enqueue_trace.py --child <lib.so> <out.txt>       one trace (JRR_* knobs from the environment)"""
import ctypes, importlib, os, subprocess, sys, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
ENVS = [{}, {'JRR_SUPPORT_FUSED': '0'}, {'JRR_SUPPORT_FUSED': '2'}, {'JRR_SUP_OVERLAP': '0'}, {'JRR_SUP_OVERLAP': '1'}, {'JRR_ADJ_CHUNKS': '3'},
        {'JRR_NSPLIT': '7', 'JRR_NVCB16': '9', 'JRR_FWD_CHUNK_CAP': '30', 'JRR_FWD_ROUND': '0'}]
if sys.argv[1] != '--child':
    libs = sys.argv[1:3]
    out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix='jrr_trace_')
    os.makedirs(out, exist_ok=True)
    stub_so = os.path.join(out, 'libhiptrace.so')
    subprocess.check_call(['g++', '-shared', '-fPIC', '-O1', '-std=c++17', os.path.join(HERE, 'hip_trace_stub.cpp'), '-o', stub_so])
    bad = 0
    for env in ENVS:
        tag = '_'.join('%s=%s' % kv for kv in sorted(env.items())) or 'default'
        texts = []
        for i, lib in enumerate(libs):
            p = os.path.join(out, '%s_%d.txt' % (tag, i))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), '--child', lib, p], env=dict(os.environ, JRR_TRACE_STUB=stub_so, **env))
            texts.append(open(p).read())
        same = texts[0] == texts[1]
        bad += not same
        print('%-70s %6d lines %6d launches  %s' % (tag, texts[1].count('\n'), texts[1].count('\nlaunch '), 'IDENTICAL' if same else 'DIFFERENT'))
    sys.exit(1 if bad else 0)
libpath, outp = sys.argv[2], sys.argv[3]
os.environ['TRACE_OUT'] = outp
stub = ctypes.CDLL(os.environ['JRR_TRACE_STUB'], mode=ctypes.RTLD_GLOBAL)
stub.stub_first_memset4.restype = ctypes.c_void_p
lib = ctypes.CDLL(libpath)
_lib = importlib.import_module('joint-regressor-refinement_amd._lib')
for name, (res, args) in _lib.SIGNATURES.items():
    f = getattr(lib, name); f.restype = res; f.argtypes = args
sm = importlib.import_module('joint-regressor-refinement_amd.smpl_model')
P = ctypes.c_void_p
def note(s): stub.stub_note(s.encode())
def ck(rc, what):
    note('%s -> %d' % (what, rc))
    if rc < 0: note('error: ' + lib.jrr_last_error().decode())
    return rc
f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
def aligned(nbytes):
    raw = np.zeros(nbytes + 256, dtype=np.uint8); off = (-raw.ctypes.data) % 256
    return raw, raw.ctypes.data + off
m = sm.synthetic_smpl(1234)
Jh = sm.default_h36m_regressor()
keep = []
def model(hinted):
    vt, sd, pd, jr, w = f32(m['v_template']), f32(m['shapedirs']), f32(m['posedirs']), f32(m['J_regressor']), f32(m['lbs_weights'])
    par = np.ascontiguousarray(np.asarray(m['parents'], dtype=np.int32))
    hv = np.ascontiguousarray(np.nonzero((Jh > 0).any(0))[0].astype(np.int32))
    raw, base = aligned(lib.jrr_model_bytes()); keep.append(raw)
    h = P()
    ck(lib.jrr_model_create_hinted(vt.ctypes.data, sd.ctypes.data, pd.ctypes.data, jr.ctypes.data, w.ctypes.data, par.ctypes.data,
                                   hv.ctypes.data if hinted else None, hv.size if hinted else 0, base, lib.jrr_model_bytes(), ctypes.byref(h)), 'model_create')
    fc = np.ascontiguousarray(np.asarray(m['faces'], dtype=np.int32))
    ck(lib.jrr_model_set_faces(h, fc.ctypes.data, fc.shape[0]), 'set_faces')
    return h
POSE, SHAPE, KEEP, FOLDED, SIL, SUPT = 1, 2, 4, 8, 16, 128
class Run:
    def __init__(self, mh, B, flags, forge=False):
        self.B = B
        n = lib.jrr_engine_workspace_bytes(B, flags)
        self.raw, ws = aligned(n)
        self.e = P()
        ck(lib.jrr_engine_create(mh, B, B, ws, n, flags, ctypes.byref(self.e)), 'engine_create B=%d flags=%d' % (B, flags))
        z = lambda *s: np.zeros(s, dtype=np.float32)
        self.J = f32(Jh).copy(); self.Jm = z(17, 6890); self.Jv = z(17, 6890); self.Js = np.zeros(1, np.int32)
        self.x = z(B, 144); self.b = z(B, 10); self.gt = z(B, 51); self.am = z(B, 154); self.av = z(B, 154); self.st = np.zeros(1, np.int32)
        self.cam = z(B, 3); self.cm = z(B, 3); self.cv = z(B, 3); self.j2d = z(B, 34); self.hist = z(64, 5)
        stub.stub_reset()
        ck(lib.jrr_engine_set_j_regressor(self.e, self.J.ctypes.data, None, None), 'set_j_regressor')
        if flags & POSE:
            self.pd = z(1840153); ck(lib.jrr_engine_set_pose_disc(self.e, self.pd.ctypes.data, None), 'set_pose_disc')
        if flags & SHAPE:
            self.sd = z(256); ck(lib.jrr_engine_set_shape_disc(self.e, self.sd.ctypes.data, None), 'set_shape_disc')
        if forge:      # what the device would have left: a support of 17 x 3 vertices that fits the lists
            flag = stub.stub_first_memset4() - 16
            I = lambda addr, n: np.ctypeslib.as_array(ctypes.cast(addr, ctypes.POINTER(ctypes.c_int32)), (n,))
            I(flag, 64)[0] = 1
            I(flag + 256, 32)[:17] = 3
            col = I(flag + 512, 17 * 128).reshape(17, 128)
            tm = I(flag + 512 + 2 * 8704, 216)
            for i in range(17):
                for k in range(3):
                    col[i, k] = (i * 3 + k) * 9; tm[col[i, k] >> 5] = 1
            cnt = (ctypes.c_int32 * 32)(); fits = ctypes.c_int32()
            ck(lib.jrr_j_support_info(self.e, cnt, ctypes.byref(fits), None), 'j_support_info fits=%d' % fits.value)
            nt, nv = ctypes.c_int32(), ctypes.c_int32()
            note('support_tiles %d %d support_vertices %d %d' % (lib.jrr_engine_support_tiles(self.e, ctypes.byref(nt)), nt.value,
                                                                 lib.jrr_engine_support_vertices(self.e, ctypes.byref(nv)), nv.value))
    def p(self, a): return a.ctypes.data
    def run(self, n): return ck(lib.jrr_refine_run(self.e, self.p(self.x), self.p(self.b), self.p(self.gt), self.p(self.am), self.p(self.av), self.p(self.st), 1e-2, n, None, None), 'refine_run %d' % n)
    def run_after(self, n): return ck(lib.jrr_refine_run_after_j_step(self.e, self.p(self.x), self.p(self.b), self.p(self.gt), self.p(self.am), self.p(self.av), self.p(self.st), 1e-2, n, None, None), 'refine_run_after_j_step %d' % n)
    def run_j(self, n, every, after=0):
        return ck(lib.jrr_refine_run_j_steps(self.e, self.p(self.x), self.p(self.b), self.p(self.gt), self.p(self.am), self.p(self.av), self.p(self.st), 1e-2, n, None, every,
                                             self.p(self.J), self.p(self.Jm), self.p(self.Jv), self.p(self.Js), 1e-2, None, None, after, None), 'refine_run_j_steps %d every %d after %d' % (n, every, after))
    def hist_on(self): ck(lib.jrr_engine_set_loss_history(self.e, self.p(self.hist), 64, 2), 'set_loss_history')
    def reproj(self): ck(lib.jrr_engine_set_reprojection(self.e, self.p(self.j2d), self.p(self.cam), self.p(self.cm), self.p(self.cv)), 'set_reprojection')
    def close(self): lib.jrr_engine_destroy(self.e); note('engine_destroy')

def op(name, *args, tag=''):
    return ck(getattr(lib, name)(*args), name + tag)
_bufs = {}
def buf(nbytes, shift=0):      # zero-filled, 256-byte aligned (+ shift); one buffer per size, shared by the calls: nothing runs
    if nbytes not in _bufs: _bufs[nbytes] = aligned(nbytes + 64)
    return _bufs[nbytes][1] + shift
def disc_ops(r, refuse):
    """the discriminator operators on engine r; refuse: the engine has neither discriminator"""
    B, t = r.B, ' refused' if refuse else ''
    x, o, g, dP, sq = buf(B * 144 * 4), buf(B * 25 * 4), buf(B * 25 * 4), buf(1840153 * 4), buf(B * 4)
    op('jrr_pose_disc_forward', r.e, x, o, None, tag=t)
    op('jrr_pose_disc_backward_input', r.e, x, 1.0, 1.0, x, None, tag=t)
    op('jrr_pose_disc_vjp_input', r.e, x, g, x, None, tag=t)
    op('jrr_pose_disc_backward_params', r.e, x, 1.0, dP, sq, None, tag=t)
    op('jrr_pose_disc_vjp_params', r.e, x, g, dP, None, tag=t)
    b = buf(B * 10 * 4)
    op('jrr_shape_disc_forward', r.e, b, sq, None, tag=t)
    op('jrr_shape_disc_vjp_input', r.e, b, sq, b, None, tag=t)
    op('jrr_shape_disc_backward_params', r.e, b, 1.0, dP, sq, None, tag=t)
    op('jrr_shape_disc_vjp_params', r.e, b, sq, dP, None, tag=t)
    op('jrr_refine_aux_losses', r.e, sq, buf(B * 4 + 4), None, tag=t)
    if refuse:
        op('jrr_engine_set_pose_disc', r.e, dP, None, tag=t); op('jrr_engine_set_shape_disc', r.e, dP, None, tag=t)
        op('jrr_pose_disc_forward', r.e, None, o, None, tag=' null')
def sil_ops(r, img, refuse):
    """the silhouette operators on engine r (img: a (B,224,224) float32 buffer); refuse: an engine without JRR_FLAG_SILHOUETTE"""
    B, t = r.B, ' refused' if refuse else ''
    v, cam = buf(B * 6890 * 3 * 4), buf(B * 3 * 4)
    op('jrr_silhouette_forward', r.e, v, cam, img, None, tag=t)
    op('jrr_silhouette_backward', r.e, img, v, cam, None, tag=t)
    op('jrr_silhouette_pix_to_face', r.e, img, None, tag=t)
    op('jrr_silhouette_loss_grad', r.e, r.p(r.x), r.p(r.b), cam, img, buf(B * 4), v, buf(B * 3 * 4 + 4), None, tag=t)
    op('jrr_engine_set_silhouette', r.e, img, None, None, None, tag=' refused')
mh, mplain = model(True), model(False)
for B in (64, 256, 1024, 4096):
    note('== support engine B=%d' % B)
    r = Run(mh, B, POSE | SHAPE | KEEP | SUPT, forge=True)
    r.run(3); r.hist_on(); r.run_j(5, 2); r.run_j(4, 2, 2); r.reproj(); r.run(2); r.run_j(3, 3, 1)
    ck(lib.jrr_engine_set_profiling(r.e, 1), 'profiling'); r.run(2); r.close()
    note('== support engine, joint loss only B=%d' % B)
    r = Run(mh, B, KEEP | SUPT, forge=True); r.run(3); r.run_j(4, 2); r.close()
for B in (64, 1024):
    note('== chain engine B=%d' % B)
    r = Run(mplain, B, POSE | SHAPE | KEEP)
    r.run(2); r.hist_on(); r.run_j(5, 2); r.run_j(4, 2, 2); r.run_j(3, 3, 1); r.reproj(); r.run(2)
    g = np.zeros((17, 6890), np.float32)
    ck(lib.jrr_j_regressor_grad(r.e, r.p(r.x), r.p(r.b), r.p(r.gt), g.ctypes.data, None, None, None), 'j_regressor_grad'); r.run_after(2)
    ck(lib.jrr_engine_set_profiling(r.e, 1), 'profiling'); r.run(2)
    note('== operators: discriminators B=%d' % B); disc_ops(r, False); r.close()
    note('== chain engine with known support B=%d' % B)
    r = Run(mplain, B, POSE | KEEP, forge=True); r.run(2); r.run_j(5, 2); r.close()
    note('== plain engine B=%d' % B)
    r = Run(mplain, B, 0); r.run(2)
    note('== operators: refused on a plain engine B=%d' % B); disc_ops(r, True); sil_ops(r, buf(16), True); r.close()
    note('== folded engine B=%d' % B)
    r = Run(mplain, B, POSE | SHAPE | KEEP | FOLDED); ck(lib.jrr_engine_set_folded(r.e, 1, None), 'set_folded'); r.hist_on(); r.run(2); r.run_j(4, 2); r.reproj(); r.run(1); r.close()
    note('== silhouette engine B=%d' % B)
    r = Run(mplain, B, POSE | KEEP | SIL)
    mask = np.zeros((B, 224, 224), np.float32)
    ck(lib.jrr_engine_set_silhouette(r.e, mask.ctypes.data, r.p(r.cam), r.p(r.cm), r.p(r.cv)), 'set_silhouette'); r.hist_on(); r.run(3); r.reproj(); r.run_j(4, 2)
    note('== operators: silhouette B=%d' % B); sil_ops(r, mask.ctypes.data, False); r.close()
note('== operators without an engine')
B, S = 2, 8
c3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
img, out, st = buf(B * 3 * S * S * 4), buf(B * 3 * S * S * 4 + 64), buf(64)
op('jrr_image_crop', buf(1024), 1024, buf(B * 64), buf(B * 16), B, None, None, S, out, 4, img, st, None)
op('jrr_image_crop', buf(1024), 1024, buf(B * 64), buf(B * 16), B, None, None, 6, out, 0, None, st, None, tag=' refused')
op('jrr_mask_prepare', buf(1024), B, S, S, out, st, None)
op('jrr_mask_prepare', buf(1024), B, 0, S, out, st, None, tag=' refused')
op('jrr_silhouette_compare', img, out, B, S, S, 0.5, 0.8, st, None)
op('jrr_silhouette_compare', img, out, B, 3, 3, 0.5, 0.8, st, None, tag=' refused')
op('jrr_fit_overlay', img, out, None, None, None, None, 0, B, S, 0.5, 0.8, 2.0, buf(B * S * S * 3), None)
op('jrr_fit_overlay', img, out, None, None, None, None, 0, B, 6, 0.5, 0.8, 2.0, buf(B * S * S * 3), None, tag=' refused')
NF = int(np.asarray(m['faces']).shape[0])
verts, nrm, faces, adj = buf(B * 6890 * 3 * 4), buf(B * 6890 * 3 * 4 + 64), buf(NF * 3 * 4), buf(NF * 3 * 4 + 64)
op('jrr_vertex_normals', verts, faces, buf(6891 * 4), adj, B, 6890, NF, nrm, None)
op('jrr_vertex_normals', verts, faces, buf(6891 * 4), adj, B, 0, NF, nrm, None, tag=' refused')
op('jrr_mesh_shade', verts, nrm, faces, buf(B * 3 * 4), buf(B * S * S * 4), None, None, None, B, 6890, NF, S, c3, 1.0, 0.3, c3, 1.0, buf(B * S * S * 3), None, None, st, None)
op('jrr_mesh_shade', verts, nrm, faces, buf(B * 3 * 4), buf(B * S * S * 4), None, None, None, B, 6890, NF, 260, c3, 1.0, 0.3, c3, 1.0, buf(B * S * S * 3), None, None, st, None, tag=' refused')
op('jrr_rotmat_to_axis_angle', buf(B * 9 * 4), buf(B * 3 * 4), B, None)
op('jrr_rotmat_to_axis_angle', buf(B * 9 * 4), buf(B * 3 * 4), -1, None, tag=' refused')
table = buf(4 * 1024)
op('jrr_pose_export', buf(B * 144 * 4), buf(B * 10 * 4), buf(B * 3 * 4), None, 0, buf(B * 8), table, 4, st, B, None)
op('jrr_pose_export', buf(B * 144 * 4), buf(B * 10 * 4), buf(B * 3 * 4), None, 11, buf(B * 8), table, 4, st, B, None, tag=' refused')
order, run_ = buf(B * 4), buf(B * 4 + 64)
op('jrr_pose_smooth', table, 4, order, run_, B, buf(17 * 4), 1, 0, B, buf(B * 144 * 4), buf(B * 10 * 4), buf(B * 3 * 4), buf(B * 4 + 128), st, None)
op('jrr_pose_smooth', table, 4, order, run_, B, buf(17 * 4), 17, 0, B, buf(B * 144 * 4), buf(B * 10 * 4), buf(B * 3 * 4), buf(B * 4 + 128), st, None, tag=' refused')
op('jrr_pose_jitter', table, 4, order, run_, B, 0, B, buf(B * 4 + 128), st, None)
op('jrr_pose_jitter', table, 4, order, run_, B, 1, B, buf(B * 4 + 128), st, None, tag=' refused')
pred, tgt, ej, epa = buf(B * 51 * 4), buf(B * 51 * 4 + 64), buf(B * 17 * 4), buf(B * 17 * 4 + 64)
op('jrr_evaluate', pred, tgt, buf(B * 4), buf(B * 4 + 64), B, None)
op('jrr_evaluate', pred, tgt, buf(B * 4), buf(B * 4 + 64), 0, None, tag=' refused')
op('jrr_evaluate_joints', pred, tgt, ej, epa, B, None)
op('jrr_evaluate_joints', pred, tgt, buf(B * 17 * 4, 4), epa, B, None, tag=' refused')
for n_reg in (1, 2):
    need = lib.jrr_regress_joints_workspace_bytes(n_reg)
    note('regress_joints_workspace_bytes %d -> %d' % (n_reg, need))
    ws, Jr = buf(need), buf(n_reg * 17 * 6890 * 4 + 64)
    op('jrr_regress_joints_prepare', Jr, n_reg, None, ws, need, None, tag=' n_reg=%d' % n_reg)
    op('jrr_regress_joints', verts, B, ws, n_reg, buf(n_reg * B * 51 * 4 + 128), None, tag=' n_reg=%d' % n_reg)
    op('jrr_regress_joints_prepare', Jr, n_reg, None, ws, need - 1, None, tag=' n_reg=%d refused' % n_reg)
note('regress_joints_workspace_bytes 0 -> %d, 5 -> %d' % (lib.jrr_regress_joints_workspace_bytes(0), lib.jrr_regress_joints_workspace_bytes(5)))
op('jrr_regress_joints', verts, B, buf(1024), 0, buf(B * 51 * 4 + 128), None, tag=' refused')
acc = buf(1 << 16)
op('jrr_eval_accumulate', ej, epa, buf(B * 4), B, 1, acc, None)
op('jrr_eval_accumulate', ej, epa, buf(B * 4), B, 0, acc, None, tag=' refused')
op('jrr_regressor_shift_accumulate', pred, tgt, None, B, 1, acc, None)
op('jrr_regressor_shift_accumulate', pred, tgt, None, B, 0, acc, None, tag=' refused')
col = (ctypes.c_uint8 * 3)(255, 0, 0)
op('jrr_draw_discs', buf(B * S * S * 3), B, S, S, buf(B * 2 * 4), None, 2.0, col, 1, 1, None)
op('jrr_draw_discs', buf(B * S * S * 3), B, S, S, buf(B * 2 * 4), None, 2.0, col, 0, 1, None, tag=' refused')
note('done')
