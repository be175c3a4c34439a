"""group_table.py: the host half of the grouped int64 accumulator, on a few small tables.  No GPU."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import PKG_NAME, ROOT

gt = importlib.import_module(f'{PKG_NAME}.group_table')

ROW = 3


def _table(rows, ignored=0, bad_group=0):
    return np.array([x for r in rows for x in r] + [ignored, bad_group], dtype=np.int64)


def _stats(row):
    return {'n': int(row[0]), 'sum': int(row[1] + row[2])}


def test_constants_are_those_of_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'jrr.h')).read()
    for name, value in (('JRR_EVAL_ACC_TRAILER', gt.TRAILER), ('JRR_EVAL_ACC_TRAILER_IGNORED', gt.T_IGNORED),
                        ('JRR_EVAL_ACC_TRAILER_BAD_GROUP', gt.T_BAD_GROUP), ('JRR_EVAL_ACC_MAX_GROUPS', gt.MAX_GROUPS)):
        assert f'{name} = {value}' in hdr, name
    er = importlib.import_module(f'{PKG_NAME}.eval_report')
    assert er.ALL == gt.ALL == 'all' and er.MAX_GROUPS == gt.MAX_GROUPS and er._rank is gt.rank and er.TRAILER == gt.TRAILER


def test_split_and_its_two_refusals_with_both_nouns():
    t = _table([[1, 2, 3], [4, 5, 6]], ignored=7)
    rows, ignored = gt.split(t, 2, ROW, 'toy table')
    assert rows.tolist() == [[1, 2, 3], [4, 5, 6]] and ignored == 7
    for wrong in (t[:-1], t.astype(np.int32), t.reshape(2, 4)):
        with pytest.raises(ValueError, match=r'toy table: 8 int64 expected for 2 groups, got '):
            gt.split(wrong, 2, ROW, 'toy table')
    with pytest.raises(ValueError, match=r'toy table: 11 int64 expected for 3 groups, got int64 \(8,\)'):
        gt.split(t, 3, ROW, 'toy table')
    bad = _table([[1, 2, 3], [4, 5, 6]], ignored=7, bad_group=2)
    with pytest.raises(RuntimeError, match=r'toy table: 2 poses carried a group id outside \[0, 2\); they were not scored'):
        gt.split(bad, 2, ROW, 'toy table')
    with pytest.raises(RuntimeError, match=r'toy table: 2 positions carried a group id outside \[0, 2\); they were not counted'):
        gt.split(bad, 2, ROW, 'toy table', 'positions', 'counted')
    with pytest.raises(RuntimeError, match=r'toy table: 2 poses carried a subject id outside \[0, 2\); they were not scored'):
        gt.split(bad, 2, ROW, 'toy table', what='subjects', ident='subject id')
    with pytest.raises(ValueError, match=r'8 int64 expected for 2 subjects'):
        gt.split(bad[:-1], 2, ROW, 'toy table', what='subjects', ident='subject id')


def test_all_is_the_sum_of_the_group_rows():
    t = _table([[1, 2, 3], [4, 5, 6], [0, 0, 0]], ignored=2)
    doc = gt.derive(t, ['a', 'b', 'empty'], ROW, _stats, 'toy table')
    assert list(doc) == ['groups', 'all', 'ignored'] and list(doc['groups']) == ['a', 'b', 'empty']
    assert doc['groups'] == {'a': {'n': 1, 'sum': 5}, 'b': {'n': 4, 'sum': 11}, 'empty': {'n': 0, 'sum': 0}}
    assert doc['all'] == {'n': 5, 'sum': 16} and doc['ignored'] == 2
    for key in ('n', 'sum'):
        assert doc['all'][key] == sum(g[key] for g in doc['groups'].values())
    with pytest.raises(RuntimeError, match='positions carried'):
        gt.derive(_table([[1, 2, 3]], bad_group=1), ['a'], ROW, _stats, 'toy table', 'positions')


def test_all_reduce_without_a_group_returns_the_same_words():
    for dtype in (torch.int64, torch.int32):
        t = torch.arange(8, dtype=dtype)
        assert gt.all_reduce(t, reduce=False) is t and gt.all_reduce(t) is t and gt.all_reduce(t, in_place=True) is t
        assert t.tolist() == list(range(8))
    assert gt.rank() == 0


def test_group_count_check():
    gt.check_groups(1)
    gt.check_groups(gt.MAX_GROUPS)
    with pytest.raises(ValueError, match=r'^0 groups: 1 \.\. 1024$'):
        gt.check_groups(0)
    with pytest.raises(ValueError, match=r'^1025 subjects: 1 \.\. 1024$'):
        gt.check_groups(gt.MAX_GROUPS + 1, 'subjects')


def test_fmt_and_arrow():
    assert gt.fmt(None) == '-' and gt.fmt(1.005, '.1f') == '1.0' and gt.fmt(2.0, '+.2f') == '+2.00'
    assert gt.arrow(1.0, None) == '1.00 → -' and gt.arrow(None, 0.25, '.3f') == '- → 0.250'


def test_write_load_round_trip_and_the_version_refusal(tmp_path):
    doc = {'layout_version': 3, 'data': gt.derive(_table([[1, 2, 3]]), ['a'], ROW, _stats, 'toy table'), 'when': np.int64(5)}
    md = lambda d: f'# toy\n\n{d["data"]["all"]["sum"]} → done\n'
    out = str(tmp_path / 'deep' / 'er')
    assert gt.write(out, 'toy', doc, md) is doc
    assert sorted(os.listdir(out)) == ['toy.json', 'toy.md']
    assert open(os.path.join(out, 'toy.md'), encoding='utf-8').read() == '# toy\n\n5 → done\n'
    text = open(os.path.join(out, 'toy.json')).read()
    assert text.startswith('{\n "data": {\n  "all": {') and '"when": "5"' in text           # indent 1, sorted keys, str() for what json cannot
    back = gt.load(out, 'toy', 3)
    assert back['data'] == doc['data'] and back['layout_version'] == 3
    with pytest.raises(ValueError, match=f'{out}: table layout version 3, this build reads version 4'):
        gt.load(out, 'toy', 4)
    with pytest.raises(ValueError, match='depth table layout version 3, this build reads version 2'):
        gt.load(out, 'toy', 2, 'depth table')
    # a document given as a function is built on the writing rank, after the directory exists
    seen = []
    made = gt.write(str(tmp_path / 'late'), 'toy', lambda: (seen.append(os.path.isdir(str(tmp_path / 'late'))), dict(doc, layout_version=9))[1], md)
    assert seen == [True] and made['layout_version'] == 9 and gt.load(str(tmp_path / 'late'), 'toy', 9)['data'] == doc['data']
