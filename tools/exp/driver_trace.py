"""Does optimize_pose_refiner() of two trees make the same calls?  Without a GPU: the driver of each tree runs under the recording
stand-in (tests/driver_standin.py of THIS tree), one fresh child process per tree and flag set; the call logs, the records (all fields
but the two timings), the returned tensors and every refined.npz / PNG written must be identical.
    python tools/exp/driver_trace.py <parent tree> <new tree>"""
import hashlib, json, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STANDIN = os.path.join(ROOT, 'tests', 'driver_standin.py')
SMALL = ['--batch_size', '6', '--inner_iters', '2', '--synthetic_batches', '2']
J1 = ['--batch_size', '6', '--inner_iters', '3', '--synthetic_batches', '2', '--j_step_every', '1']


def write_dataset(root, n, seed, images=False):
    """precomputed_val/ in the reference layout with 6-D poses (as tests/test_refined_export.py writes it); images: .npy frames and
    224 x 224 masks beside it (as tests/test_gpu_image_pipeline.py does)"""
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    g = torch.Generator().manual_seed(seed)
    files = dict(bboxes=torch.tensor([[20., 10., 120., 100.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 100,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))
    rng = np.random.RandomState(seed)
    for i in range(n if images else 0):
        np.save(os.path.join(loc, f'frame_{i:06d}.npy'), rng.randint(0, 256, (120, 160, 3)).astype(np.uint8))
        np.save(os.path.join(loc, f'mask_{i:06d}.npy'), (rng.randint(0, 2, (224, 224)) * 255).astype(np.uint8))


def cases(tmp):
    """(name, flags with {out} for the tree's own output directory, one-rank gloo group?)"""
    plain, pics = os.path.join(tmp, 'data40'), os.path.join(tmp, 'data10img')
    write_dataset(plain, 40, 3)
    write_dataset(pics, 10, 4, images=True)
    ds = ['--batch_size', '16', '--inner_iters', '2', '--data_root', plain]
    return [('defaults', SMALL, False), ('--all_vertex_tiles', SMALL + ['--all_vertex_tiles'], False),
            ('--shape_disc --reprojection --silhouette', SMALL + ['--shape_disc', '--reprojection', '--silhouette', '--camera_iters', '5'], False),
            ('--no_pose_disc', SMALL + ['--no_pose_disc'], False), ('--j_step_every 1', J1, False),
            ('--j_step_every 1, gloo, --j_allreduce support', J1 + ['--j_allreduce', 'support'], True),
            ('--j_step_every 1, gloo, --j_allreduce dense', J1 + ['--j_allreduce', 'dense'], True),
            ('--silhouette --fit_report', SMALL + ['--silhouette', '--fit_report', '{out}/fit'], False),
            ('--save_refined', SMALL + ['--save_refined', '{out}/ref'], False),
            ('--silhouette --fit_report --save_refined', SMALL + ['--silhouette', '--fit_report', '{out}/fit2', '--save_refined', '{out}/ref2'], False),
            ('dataset 40 @ 16 (ragged 8)', ds, False), ('dataset 40 @ 16 --save_refined', ds + ['--save_refined', '{out}/table'], False),
            ('dataset 40 @ 16 --init_refined', ds + ['--init_refined', '{out}/table'], False),
            ('dataset 10 @ 6 --silhouette --image_masks --fit_report',
             ['--batch_size', '6', '--inner_iters', '2', '--data_root', pics, '--silhouette', '--image_masks', '--fit_report', '{out}/fit3'], False)]


def child(tree, out, k, flags, group):
    path = os.path.join(out, f'case{k:02d}.json')
    env = dict(os.environ, OMP_NUM_THREADS='2', JRR_DIST_SINGLE_RANK='1' if group else '0')
    r = subprocess.run([sys.executable, '-W', 'ignore', STANDIN, tree, path] + [f.replace('{out}', out) for f in flags], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {'error': r.stderr[-1500:]}
    with open(path) as f:
        return json.load(f)


def written(out):
    """sha256 of every refined.npz array set and PNG under `out` (meta.json quotes the flags, so the directory names)"""
    sums = {}
    for base, _, names in os.walk(out):
        for name in sorted(names):
            if name.endswith(('.png', '.npz')):
                with open(os.path.join(base, name), 'rb') as f:
                    sums[os.path.relpath(os.path.join(base, name), out)] = hashlib.sha256(f.read()).hexdigest()[:16]
    return sums


def main():
    trees = [os.path.abspath(p) for p in sys.argv[1:3]]
    with tempfile.TemporaryDirectory() as tmp:
        todo = cases(tmp)
        outs = [os.path.join(tmp, f'tree{i}') for i in range(2)]
        for o in outs:
            os.makedirs(o)
        # the --init_refined case reads the table its own tree's --save_refined case wrote: the cases of a tree run in order
        with ThreadPoolExecutor(max_workers=2) as ex:
            got = list(ex.map(lambda i: [child(trees[i], outs[i], k, f, g) for k, (_, f, g) in enumerate(todo)], range(2)))
        files = [written(o) for o in outs]
    print(f'{"flag set":58s} {"calls":>5s}  log        records + return value')
    bad = 0
    for (name, _, _), a, b in zip(todo, *got):
        if 'error' in a or 'error' in b:
            print(f'{name:58s} FAILED\n{a.get("error", "")}{b.get("error", "")}')
            bad += 1
            continue
        same_log, same_res = a['log'] == b['log'], json.dumps(a['result']) == json.dumps(b['result'])      # (key order too)
        bad += not (same_log and same_res)
        print(f'{name:58s} {len(b["log"]):5d}  {"IDENTICAL" if same_log else "DIFFERENT":9s}  {"IDENTICAL" if same_res else "DIFFERENT"}')
        if not same_log:
            first = next((i for i, (x, y) in enumerate(zip(a['log'], b['log'])) if x != y), min(len(a['log']), len(b['log'])))
            print('   first difference:\n   ' + '\n   '.join(log[first] if first < len(log) else '(end)' for log in (a['log'], b['log'])))
    same_files = files[0] == files[1]
    print(f'files written (refined.npz, PNG): {len(files[1])}, {"IDENTICAL" if same_files else "DIFFERENT"}')
    print(f'{len(todo)} flag sets, {bad} different')
    sys.exit(1 if bad or not same_files else 0)


if __name__ == '__main__':
    main()
