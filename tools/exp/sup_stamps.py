"""Phase stamps of the composed support-vertex kernel k_sup_step (chain.hip, supk.h): workgroup 0's phase boundaries on the 100 MHz
counter.  The shipped library carries no stamps: this script builds tools/probe/libjrr_supstamp.so (build_variant.py: the shipped
kernel + wall_clock64() stamps into a device symbol, read back through jrr_debug_read), loads it through JRR_LIB and prints them.

usage: python tools/exp/sup_stamps.py --build-only        (cross-compiles the variant library, no GPU)
       python tools/exp/sup_stamps.py [B] [pose_disc 0/1]   (GPU box; builds the variant first if it is not there)"""
import ctypes
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
VARIANT = os.path.join(ROOT, 'tools', 'probe', 'libjrr_supstamp.so')

# (old, new) text pairs: k_sup_step<0> stamps g_dbg[0..5], its support body g_dbg[8..13]
BODY = ['  // ---- v_posed = Ds . F', '  // ---- skinning: T = sum_j', '  // ---- joints (ascending vertex row)',
        '  // ---- vertex adjoint dverts = Jn^T dj', '  // ---- dA_j = sum_v W[v,j]', '  // ---- dF = Ds^T . dvp']
PAIRS = [
    'supk.h:__device__ __forceinline__ void sup_body(float* __restrict__ lds, int blk, const SupArgs& a) {\n',
    '__device__ long long g_dbg[32];\n'
    '__device__ __forceinline__ void sup_body(float* __restrict__ lds, int blk, const SupArgs& a, bool stamps = false) {\n'
    '  auto stamp = [&](int i) { if (stamps && blockIdx.x == 0 && threadIdx.x == 0) g_dbg[8 + i] = wall_clock64(); };\n',
]
for i, anchor in enumerate(BODY):
    PAIRS += ['supk.h:' + anchor, f'  stamp({i});\n' + anchor]
PAIRS += [
    'template <int PHASE>\n__global__ __launch_bounds__(SUP_THREADS) void k_sup_step(',
    'extern "C" void jrr_debug_read(long long* out) { (void)hipDeviceSynchronize(); (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(long long) * 32); }\n'
    'template <int PHASE>\n__global__ __launch_bounds__(SUP_THREADS) void k_sup_step(',
    '  const int blk = blockIdx.x, B = a.sup.B, BP = a.sup.BP;\n',
    '  const int blk = blockIdx.x, B = a.sup.B, BP = a.sup.BP;\n'
    '  auto stamp = [&](int i) { if (PHASE == 0 && blockIdx.x == 0 && threadIdx.x == 0) g_dbg[i] = wall_clock64(); };\n  stamp(0);\n',
    '    sup_body(pool, blk, a.sup);\n',
    '    stamp(1);\n    sup_body(pool, blk, a.sup, PHASE == 0);\n',
    '    // (the per-joint MLP adjoint closed the support body: one interleaved pair of joints per wave, supk.h)\n',
    '    stamp(2);\n    // (the per-joint MLP adjoint closed the support body: one interleaved pair of joints per wave, supk.h)\n    stamp(3);\n',
    '    // (the image the support body staged',
    '    stamp(4);\n    // (the image the support body staged',
    '  __syncthreads();\n}\n\nint launch_sup_step(',
    '  __syncthreads();\n  stamp(5);\n}\n\nint launch_sup_step(',
]


def build_variant():
    subprocess.check_call([sys.executable, os.path.join(HERE, 'build_variant.py'), 'supstamp', 'chain.hip'] + PAIRS)


def main():
    args = [a for a in sys.argv[1:] if a != '--build-only']
    if '--build-only' in sys.argv[1:]:
        build_variant()
        return
    if not os.path.exists(VARIANT):
        build_variant()
    os.environ['JRR_LIB'] = VARIANT          # before the package loads its library
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    PKG = 'joint-regressor-refinement_amd'
    B = int(args[0]) if len(args) > 0 else 4096
    pd = int(args[1]) if len(args) > 1 else 1
    dev = torch.device('cuda:0')
    sm = importlib.import_module(PKG + '.smpl_model')
    em = importlib.import_module(PKG + '.engine')
    lib = ctypes.CDLL(VARIANT)          # the handle the package holds: one copy of g_dbg
    model = sm.synthetic_smpl(1234)
    J_np = sm.default_h36m_regressor()
    batch = sm.synthetic_batch(model, J_np, B, seed=5)
    dm = em.DeviceModel(model, dev, hint_vertices=np.nonzero((J_np > 0).any(0))[0])
    eng = em.RefineEngine(dm, B, flags=em.FLAG_KEEP_VERTS | em.FLAG_SUPPORT_TILES | (em.FLAG_POSE_DISC if pd else 0))
    J = torch.from_numpy(J_np).to(dev).clone()
    eng.set_j_regressor(J)
    if pd:
        eng.set_pose_disc(torch.randn(1840153, device=dev) * 0.02)
    print('support', eng.j_support_info()[1], eng.support_tiles())
    x = torch.from_numpy(batch['pose6d']).to(dev).contiguous()
    b = torch.from_numpy(batch['betas']).to(dev).contiguous()
    gt = torch.from_numpy(batch['gt_j3d']).to(dev)
    gt = (gt - gt[:, :1]).contiguous()
    m, v = torch.zeros(B, 154, device=dev), torch.zeros(B, 154, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    acc = np.zeros(32)
    n = 0
    buf = (ctypes.c_longlong * 32)()
    for rep in range(20):
        eng.refine_run(x, b, gt, m, v, st, 1e-2, 5)
        lib.jrr_debug_read(buf)          # (synchronises the device)
        s = np.array(buf[:], dtype=np.float64)
        if rep >= 5:
            acc += s - s[0]
            n += 1
    acc /= n
    names = ['start', 'chain forward', 'support fwd+bwd + per-joint MLP adjoint (one interleaved pair of joints per wave)', '(nothing)', 'chain adjoint + Adam', 'per-joint MLP forward x2 (end)']
    print('k_sup_step, workgroup 0, us since its start:')
    for i in range(1, 6):
        print(f'  {names[i]:100s} ends at {acc[i] / 100:8.2f}   (+{(acc[i] - acc[i - 1]) / 100:6.2f})')
    sub = ['operands + MLP image -> LDS', 'v_posed = Ds F (matrix)', 'skinning', 'joints + loss', 'dverts, dvp', 'dA (then dF = Ds^T dvp and the MLP adjoint pairs follow)']
    print('inside the support body (us since the kernel start):')
    for i in range(6):
        print(f'  {sub[i]:70s} ends at {acc[8 + i] / 100:8.2f}')


if __name__ == '__main__':
    main()
