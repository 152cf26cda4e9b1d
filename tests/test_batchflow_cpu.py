"""Host logic the batch workflows share (nadavca_amd/batchflow.py, no GPU): the segment index against a plain
loop, the one policy for per-read kernel status on hand-made status arrays (numpy and torch CPU), the loaders."""
import numpy as np
import pytest


def _seg_index_loop(off):
    owner, inner = [], []
    for s in range(len(off) - 1):
        for p in range(off[s + 1] - off[s]):
            owner.append(s)
            inner.append(p)
    return owner, inner


@pytest.mark.parametrize('off', [[0], [0, 0], [0, 0, 3, 3, 5, 5], [0, 4], [0, 2, 3, 7]])
@pytest.mark.parametrize('give_total', [False, True])
def test_seg_index_equals_a_plain_loop(off, give_total):
    import torch
    from nadavca_amd.batchflow import seg_index
    t = torch.tensor(off, dtype=torch.int64)
    owner, inner = seg_index(t, off[-1]) if give_total else seg_index(t)
    assert owner.dtype == torch.int64 and inner.dtype == torch.int64
    assert owner.shape == (off[-1],) and inner.shape == (off[-1],)
    exp_owner, exp_inner = _seg_index_loop(off)
    assert owner.tolist() == exp_owner and inner.tolist() == exp_inner


def test_seg_index_on_the_case_the_workflows_rely_on():
    import torch
    from nadavca_amd.batchflow import seg_index
    owner, inner = seg_index(torch.tensor([0, 0, 3, 3, 5, 5], dtype=torch.int64))
    assert owner.tolist() == [1, 1, 1, 3, 3] and inner.tolist() == [0, 1, 2, 0, 1]


def _forms(values):
    import torch
    a = np.array(values, dtype=np.int32)
    return [a, torch.from_numpy(a.copy())]


def _indices(values):
    import torch
    a = np.array(values, dtype=np.int64)
    return [a, torch.from_numpy(a.copy())]


BAD, BAND, WIDE = -1, -2, -3     # _lib.READ_BAD_INPUT, READ_BAD_BAND, READ_TOO_WIDE


def test_status_codes_are_the_library_s():
    from nadavca_amd import _lib
    assert (_lib.READ_BAD_INPUT, _lib.READ_BAD_BAND, _lib.READ_TOO_WIDE) == (BAD, BAND, WIDE)


@pytest.mark.parametrize('too_wide', ['raise', 'skip', 'invalid'])
def test_check_status_is_silent_without_a_negative_status(too_wide, capsys):
    from nadavca_amd.batchflow import check_status
    for status in _forms([0, 1, 0, 1]) + _forms([]):
        assert check_status('op', status, too_wide=too_wide) is None
    assert capsys.readouterr() == ('', '')


def test_check_status_invalid_input_names_the_first_eight_reads():
    from nadavca_amd.batchflow import check_status
    values = [0, BAD, 1, BAND] + [BAD] * 10
    for status in _forms(values):
        for too_wide in ('raise', 'skip'):
            with pytest.raises(ValueError) as e:
                check_status('refine_alignment', status, too_wide=too_wide)
            assert str(e.value) == ('refine_alignment: invalid input for read(s) [1, 3, 4, 5, 6, 7, 8, 9] '
                                    '(status [-1, -2, -1, -1, -1, -1, -1, -1])')
        # the batch forms name the reads by their index in the ReadBatch
        for live in _indices(np.arange(len(values)) * 10 + 5):
            with pytest.raises(ValueError) as e:
                check_status('refine_alignment', status, live, too_wide='skip')
            assert str(e.value) == ('refine_alignment: invalid input for read(s) [15, 35, 45, 55, 65, 75, 85, 95] '
                                    '(status [-1, -2, -1, -1, -1, -1, -1, -1])')


def test_check_status_too_wide_raises_the_library_s_error(capsys):
    from nadavca_amd._lib import NadavcaHipError
    from nadavca_amd.batchflow import check_status
    for status in _forms([0, WIDE, 1] + [WIDE] * 9):
        with pytest.raises(NadavcaHipError) as e:
            check_status('estimate_log_likelihoods', status)
        assert not isinstance(e.value, ValueError)
        assert str(e.value) == ('estimate_log_likelihoods: the band of read(s) [1, 3, 4, 5, 6, 7, 8, 9] is wider than '
                                'the compiled kernels serve (INTEGRATION.md, limits)')
    assert capsys.readouterr() == ('', '')


def test_check_status_too_wide_is_skipped_with_a_note_by_the_batch_forms(capsys):
    """a too-wide read no longer aborts the batch workflows."""
    from nadavca_amd.batchflow import check_status
    values = [0, WIDE, 1] + [WIDE] * 9
    for status in _forms(values):
        for live in _indices(np.arange(len(values)) + 100):
            assert check_status('estimate_log_likelihoods', status, live, too_wide='skip') is None
            out, err = capsys.readouterr()
            assert out == ''
            assert err == ('estimate_log_likelihoods: 10 read(s) skipped, band wider than the compiled kernels serve '
                           '(first: [101, 103, 104, 105, 106, 107, 108, 109])\n')
    assert status.tolist() == values        # the read stays in the status, as one without a path does


def test_check_status_invalid_wins_over_too_wide(capsys):
    from nadavca_amd.batchflow import check_status
    for status in _forms([WIDE, 0, BAND, WIDE]):
        for too_wide in ('raise', 'skip'):
            with pytest.raises(ValueError) as e:
                check_status('op', status, too_wide=too_wide)
            assert str(e.value) == 'op: invalid input for read(s) [2] (status [-2])'
    assert capsys.readouterr() == ('', '')


def test_check_status_of_refine_and_renormalize_keeps_its_value_error():
    """ProbabilityEstimator.refine_and_renormalize reports every negative status, a too-wide band included, as
    invalid input (ValueError, not NadavcaHipError) and without the codes."""
    from nadavca_amd.batchflow import check_status
    for status in _forms([0, WIDE, 1, BAD] + [WIDE] * 8):
        with pytest.raises(ValueError) as e:
            check_status('refine_alignment', status, too_wide='invalid')
        assert str(e.value) == 'refine_alignment: invalid input for read(s) [1, 3, 4, 5, 6, 7, 8, 9]'


def test_loaders_pass_objects_through_and_read_paths(tmp_path):
    import importlib
    import pathlib
    from nadavca_amd import defaults
    from nadavca_amd.batchflow import load_config, load_kmer_model
    cfg = {'bandwidth': 7}
    assert load_config(cfg) is cfg
    loaded = load_config(defaults.CONFIG_FILE)
    assert isinstance(loaded, dict) and 'bandwidth' in loaded
    assert load_config(pathlib.Path(defaults.CONFIG_FILE)) == loaded
    # (the name bench.py imports; the package re-exports the function under the module's name)
    assert importlib.import_module('nadavca_amd.align_signal')._load_config is load_config
    with pytest.raises(FileNotFoundError):
        load_config(str(tmp_path / 'missing.yaml'))
    model = object()
    assert load_kmer_model(model) is model
    for missing in (str(tmp_path / 'missing.npz'), tmp_path / 'missing.npz'):
        with pytest.raises(FileNotFoundError):
            load_kmer_model(missing)
