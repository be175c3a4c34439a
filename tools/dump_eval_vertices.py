#!/usr/bin/env python3
"""Write an `--eval_vertices` directory from the batches the evaluation report itself runs on, through this library's SMPL forward:

    python tools/dump_eval_vertices.py OUT_DIR [driver flags: --synthetic, --data_root, --batch_size, --synthetic_batches, --seed ...]
    python main.py --eval_vertices OUT_DIR --eval_report out/eval [the same flags]

OUT_DIR/vertices.npy (N,6890,3) float32 metres in SMPL vertex order, OUT_DIR/gt_j3d.npy (N,17,3) float32 mm, and OUT_DIR/paths.txt
(one frame path per mesh) when the dataset split lists its frames.  It is the template for other models: write the same three files
from their vertices (VIBE, MEVA, METRO: /root/reference/scripts/test.py:141-301,362-373) and the second command evaluates both
regressors on them.  The arrays are written through numpy's open_memmap, batch by batch.

    python tools/dump_eval_vertices.py OUT_DIR --gt_refined PATH --data_root ROOT [...]
    python main.py --eval_vertices OUT_DIR --eval_report out/eval --eval_pve [...]

`--gt_refined PATH` (a `--save_refined` directory, or one of its .npz tables: the smoothed or the fused one) also writes
OUT_DIR/gt_vertices.npy (N,6890,3) float32 metres for `--eval_pve`: the SMPL forward of `pose6d` / `shape` of the table's row at each
emitted sample's dataset index.  Samples whose row holds no refined pose (has_refined == 0) are dropped from EVERY file, so the files
keep the same rows.

`--placed` (with `--gt_refined PATH/refined_placed.npz`, the table `--place_refined` wrote): also OUT_DIR/trans.npy (N,3) float64 metres, the
camera-frame translation of each emitted sample -- vertices + trans stand in the sample's real camera.  Every other file keeps its bytes."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'


def main(argv):
    out, flags = argv[0], list(argv[1:])
    gt_refined = None
    if '--gt_refined' in flags:
        at = flags.index('--gt_refined')
        if at + 1 >= len(flags):
            raise SystemExit('--gt_refined needs a path')
        gt_refined = flags[at + 1]
        del flags[at:at + 2]
    placed = '--placed' in flags
    if placed:
        flags.remove('--placed')
        if gt_refined is None:
            raise SystemExit('--placed needs --gt_refined PATH: the table that holds trans')
    argsmod = importlib.import_module(PKG + '.args')
    argsmod._LazyArgs._ns = argsmod.get_args(flags)
    args = argsmod.args
    engine = importlib.import_module(PKG + '.engine')
    evaluation = importlib.import_module(PKG + '.test')
    sm = importlib.import_module(PKG + '.smpl_model')
    jdata = importlib.import_module(PKG + '.data')
    SMPL = importlib.import_module(PKG + '.smpl').SMPL
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    smpl = SMPL(args.smpl_dir, batch_size=1, allow_synthetic=args.synthetic or args.smpl_dir == 'SPIN/data/smpl').to(device)
    J_np = sm.default_h36m_regressor(args.j_regressor_init,
                                     allow_default=args.synthetic or args.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
    paths = jdata.split_image_paths(jdata.split_location('validation', args.data_root)) if args.data_root else None
    table = None
    if gt_refined is not None:
        if not args.data_root:
            raise SystemExit('--gt_refined needs --data_root: the table\'s rows are dataset indices')
        table = importlib.import_module(PKG + '.refined').load_path(gt_refined)
        if placed and 'trans' not in table:
            raise SystemExit(f'--placed: {gt_refined} holds no trans (python main.py --place_refined writes refined_placed.npz)')
    verts, gts, kept, gt_verts, trans = [], [], [], [], []
    engines = {}
    with torch.no_grad():
        for batch in evaluation.validation_batches(smpl.model_np, J_np, device, with_index=paths is not None or table is not None):
            B = int(batch['pose6d'].shape[0])
            if B not in engines:
                engines[B] = engine.RefineEngine(smpl.device_model, B, flags=engine.FLAG_KEEP_VERTS)
                engines[B].set_j_regressor(torch.from_numpy(J_np).float().to(device))
            _, v = engines[B].find_joints_forward(batch['betas'].to(device).float().contiguous(),
                                                  x6d=batch['pose6d'].to(device).float().contiguous(), return_verts=True)
            v, gt, index = v.cpu().numpy(), batch['gt_j3d'].float().numpy(), None if batch.get('index') is None else np.asarray(batch['index'])
            if table is not None:
                if index.max() >= table['has_refined'].shape[0]:
                    raise SystemExit(f'{gt_refined}: {table["has_refined"].shape[0]} rows, the split has a sample {int(index.max())}')
                _, g = engines[B].find_joints_forward(torch.from_numpy(table['shape'][index]).to(device).float().contiguous(),
                                                      x6d=torch.from_numpy(table['pose6d'][index]).to(device).float().contiguous(),
                                                      return_verts=True)
                has = table['has_refined'][index].astype(bool)
                v, gt, index = v[has], gt[has], index[has]
                gt_verts.append(g.cpu().numpy()[has])
                if placed:
                    trans.append(table['trans'][index])
            verts.append(v)
            gts.append(gt)
            if paths is not None:
                kept += [paths[int(i)] for i in index]
    if not verts:
        raise SystemExit('no validation batch (drop_last=True needs at least --batch_size samples)')
    N = sum(v.shape[0] for v in verts)
    os.makedirs(out, exist_ok=True)
    for name, pieces in (('vertices.npy', verts), ('gt_vertices.npy', gt_verts if table is not None else None)):
        if pieces is None:
            continue
        vm = np.lib.format.open_memmap(os.path.join(out, name), mode='w+', dtype=np.float32, shape=(N, 6890, 3))
        at = 0
        for v in pieces:
            vm[at:at + v.shape[0]] = v
            at += v.shape[0]
        vm.flush()
        del vm
    np.save(os.path.join(out, 'gt_j3d.npy'), np.concatenate(gts).astype(np.float32))
    if placed:
        np.save(os.path.join(out, 'trans.npy'), np.concatenate(trans).astype(np.float64))
    if paths is not None:
        with open(os.path.join(out, 'paths.txt'), 'w') as f:
            f.write(''.join(p + '\n' for p in kept))
    print(f'wrote {N} meshes to {out}')


if __name__ == '__main__':
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    main(sys.argv[1:])
