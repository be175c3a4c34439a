"""The ordering rules of optimize_pose_refiner(), checked on the CPU: the real driver runs under the recording stand-in
(driver_standin.py) at batch 6, 2 inner iterations, 2 synthetic batches, and the tests read the log of the calls it made."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import driver_standin as ds

SMALL = ('--batch_size', '6', '--inner_iters', '2', '--synthetic_batches', '2')
J1 = ('--batch_size', '6', '--inner_iters', '3', '--synthetic_batches', '2', '--j_step_every', '1')
BUCKET = 7829564          # bytes of the outer step's bucket with the pose discriminator on: (17 * 6890 + 1 840 153, padded) + 10 + 5 floats
# engine calls that overwrite the state of the engine's most recent forward, and the ones that read it
WRITERS = {'find_joints_forward', 'silhouette_forward', 'camera_prefit', 'refine_run', 'refine_run_j_steps', 'j_regressor_grad',
           'j_regressor_grad_support', 'j_step_apply', 'j_step_apply_support', 'set_j_regressor', 'set_pose_disc', 'set_shape_disc'}
READERS = {'find_joints_after_j_step', 'refine_aux_losses'}
FIT_ONLY = {'project_joints', 'silhouette_compare', 'fit_overlay'}
EXPORT_ONLY = {'pose_export', 'arange'}


@functools.lru_cache(maxsize=None)
def _run(flags, group=False):
    return ds.run(list(flags), one_rank_group=group)


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    """one output directory for the module, so that tests asking for the same flags share one run"""
    return tmp_path_factory.mktemp('driver_steps')


def _name(line):
    return line.split()[1]


def _per_batch(log):
    """the log's lines by outer batch: each starts where its engine is prepared and ends with the bucket's read-back; + what follows"""
    starts = [i for i, l in enumerate(log) if _name(l) == 'set_batch_norm']
    ends = [i for i, l in enumerate(log) if _name(l) == 'read_back']
    assert len(starts) == len(ends) == 2
    return [log[s:e + 1] for s, e in zip(starts, ends)], log[ends[-1] + 1:]


def _at(lines, name, nth=0):
    return [i for i, l in enumerate(lines) if _name(l) == name][nth]


def _reduced(lines):
    return [int(re.search(r'nbytes=(\d+)', l).group(1)) for l in lines if _name(l) == 'all_reduce_sum_']


def _reads_forward(line):
    return _name(line) in READERS or (_name(line) == 'refine_run' and 'after_j_step=True' in line)


def _image_dataset(root, n):
    """precomputed_val/ with 6-D poses, .npy frames and 224 x 224 masks"""
    loc = os.path.join(root, 'precomputed_val')
    os.makedirs(loc)
    g = torch.Generator().manual_seed(4)
    files = dict(bboxes=torch.tensor([[20., 10., 120., 100.]]).repeat(n, 1), betas=torch.randn(n, 10, generator=g),
                 estimated_translation=torch.randn(n, 3, generator=g), gt_j2d=torch.rand(n, 17, 2, generator=g) * 100,
                 gt_j3d=torch.randn(n, 17, 3, generator=g) * 300, intrinsics=torch.eye(3).repeat(n, 1, 1),
                 orient=torch.randn(n, 1, 6, generator=g), pose=torch.randn(n, 23, 6, generator=g))
    for k, v in files.items():
        torch.save(v, os.path.join(loc, f'{k}.pt'))
    rng = np.random.RandomState(4)
    for i in range(n):
        np.save(os.path.join(loc, f'frame_{i:06d}.npy'), rng.randint(0, 256, (120, 160, 3)).astype(np.uint8))
        np.save(os.path.join(loc, f'mask_{i:06d}.npy'), (rng.randint(0, 2, (224, 224)) * 255).astype(np.uint8))


@pytest.mark.parametrize('case', ['plain', 'fit_report', 'image_masks'])
def test_one_bucket_all_reduce_and_one_read_back_per_batch(case, tmp_path, out):
    if case == 'image_masks':
        _image_dataset(str(tmp_path), 10)
        flags = ('--batch_size', '6', '--inner_iters', '2', '--data_root', str(tmp_path), '--silhouette', '--image_masks',
                 '--fit_report', str(tmp_path / 'fit'))
    else:
        flags = SMALL + (('--silhouette', '--fit_report', str(out / 'fit')) if case == 'fit_report' else ())
    _, log = _run(flags)
    batches, rest = _per_batch(log)
    want = {'plain': [BUCKET], 'fit_report': [BUCKET, 32], 'image_masks': [4, BUCKET, 32]}[case]
    for lines in batches:
        assert _reduced(lines) == want
        assert [l for l in lines if _name(l) == 'read_back'] == lines[-1:] and '[(15,):float32]' in lines[-1]
    assert _reduced(rest) == [8]                  # the last batch's after-the-J-step sums


def test_joints_after_the_j_step_precede_the_discriminator_uploads():
    _, log = _run(SMALL + ('--shape_disc',))
    for lines in _per_batch(log)[0]:
        apply, joints = _at(lines, 'j_step_apply'), _at(lines, 'find_joints_after_j_step')
        assert apply < joints and not [l for l in lines[apply + 1:joints] if _name(l) in WRITERS]
        loop = _at(lines, 'refine_run')
        uploads = [i for i, l in enumerate(lines) if _name(l) in ('set_pose_disc', 'set_shape_disc', 'adam_step') and i > loop]
        assert len(uploads) == 4 and min(uploads) > joints


def test_fit_report_renders_sit_where_nothing_reads_them_over(out):
    _, log = _run(SMALL + ('--silhouette', '--fit_report', str(out / 'fit')))
    for lines in _per_batch(log)[0]:
        before, after = _at(lines, 'project_joints', 0), _at(lines, 'project_joints', 1)
        for p in (before, after):             # a render is three calls: the forward with vertices, the rasteriser, the projection
            assert [_name(l) for l in lines[p - 2:p + 1]] == ['find_joints_forward', 'silhouette_forward', 'project_joints']
            assert 'return_verts=True' in lines[p - 2]
        term_on = next(i for i, l in enumerate(lines) if _name(l) == 'set_silhouette' and '[None' not in l)
        assert before < term_on < _at(lines, 'refine_run')
        assert after - 2 > _at(lines, 'find_joints_after_j_step')
        assert not [l for l in lines[after + 1:] if _reads_forward(l)]


def test_refined_index_is_on_the_device_ahead_of_the_loop(out):
    _, log = _run(SMALL + ('--save_refined', str(out / 'ref')))
    for lines in _per_batch(log)[0]:
        start = int(lines[0].split()[0])
        export = lines[_at(lines, 'pose_export')]
        made = int(re.search(r'index_created_at=(\d+)', export).group(1))
        assert start < made < start + _at(lines, 'refine_run')


def test_features_that_are_off_make_no_call(out):
    strip = lambda lines: [l.split(' ', 1)[1] for l in lines]
    _, plain = _run(SMALL)
    assert not [l for l in plain if _name(l) in FIT_ONLY | EXPORT_ONLY] and _reduced(plain) == [BUCKET, BUCKET, 8]
    # --save_refined: its own lines taken out, the plain run is left, line for line
    _, saving = _run(SMALL + ('--save_refined', str(out / 'ref')))
    own = [l for l in saving if _name(l) in EXPORT_ONLY]
    assert len(own) == 4 and _reduced(saving)[-1] == (12 * 240 + 4) * 4
    assert strip(l for l in saving[:-1] if l not in own) == strip(plain)
    # --fit_report: the same against the run with the silhouette term alone
    _, sil = _run(SMALL + ('--silhouette',))
    _, fit = _run(SMALL + ('--silhouette', '--fit_report', str(out / 'fit')))
    renders = [i for i, l in enumerate(fit) if _name(l) == 'project_joints']
    own = {i - k for i in renders for k in (1, 2)} | {i for i, l in enumerate(fit) if _name(l) in FIT_ONLY or 'nbytes=32 ' in l}
    assert len(renders) == 4 and strip(l for i, l in enumerate(fit) if i not in own) == strip(sil)


def test_in_loop_j_steps_take_the_shape_the_process_group_asks_for():
    loop = lambda lines: [l for l in lines if _name(l).startswith(('refine_run', 'j_regressor_grad_', 'j_step_apply_', 'all_reduce'))
                          and f'nbytes={BUCKET}' not in l]
    _, log = _run(J1)                     # one process: ONE C call with the J steps inside, then the last iteration
    for lines in _per_batch(log)[0]:
        a, b = loop(lines)
        assert _name(a) == 'refine_run_j_steps' and 'n_iters=2 j_every=1' in a
        assert _name(b) == 'refine_run' and 'n_iters=1 after_j_step=True' in b
    _, log = _run(J1, True)               # a process group: iteration / exchange pairs, then the last iteration
    pair = ['refine_run', 'j_regressor_grad_support', 'all_reduce_sum_', 'j_step_apply_support']
    for lines in _per_batch(log)[0]:
        calls = loop(lines)
        assert [_name(l) for l in calls] == pair * 2 + ['refine_run']
        assert ['after_j_step=True' in l for l in calls if _name(l) == 'refine_run'] == [False, True, True]
        assert all('nbytes=8704' in l for l in calls if _name(l) == 'all_reduce_sum_')


RECORD = ['batch', 'joint_loss', 'pose_discriminated_loss', 'shape_discriminated_loss', 'pose_discriminator_loss', 'shape_discriminator_loss',
          'j_regressor_error', 'loss_history', 'seconds', 'seconds_batch', 'vertex_tiles_run', 'support_vertices_run', 'body_model', 'data']
AFTER = ['mpjpe', 'pampjpe', 'mpjpe difference', 'pampjpe difference']
RETURNED = ['history', 'J_regressor', 'disc_flat', 'sdisc_flat', 'x6d', 'betas', 'cam', 'shard']


def test_record_and_return_value_keys(out):
    res, _ = _run(SMALL)
    assert list(res) == RETURNED and [list(r) for r in res['history']] == [RECORD + AFTER] * 2
    assert [r['batch'] for r in res['history']] == [0, 1]
    res, _ = _run(SMALL + ('--silhouette',))
    assert list(res) == RETURNED and list(res['history'][1]) == RECORD + ['masks', 'masks_invalid'] + AFTER
    res, _ = _run(SMALL + ('--silhouette', '--fit_report', str(out / 'fit2'), '--save_refined', str(out / 'ref2')))
    assert list(res) == RETURNED + ['fit_report', 'index'] and res['index'] is None
    assert list(res['history'][1]) == RECORD + ['masks', 'masks_invalid', 'silhouette_iou_before', 'silhouette_iou_after',
                                               'j2d_error_px_before', 'j2d_error_px_after'] + AFTER
    assert list(res['fit_report']) == ['iou_before', 'iou_after', 'shard'] and res['fit_report']['shard'] == (0, 6)
