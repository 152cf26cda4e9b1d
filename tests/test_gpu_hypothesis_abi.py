"""The raw C ABI of the three listed-hypothesis entry points (nvk_estimate_hypotheses_batch_dev,
nvk_estimate_joint_hypotheses_batch_dev, nvk_estimate_edit_hypotheses_batch_dev), called through ``_lib.load()``: the
refusals their shared prologue makes before any launch — return code and the exact ``nvk_last_error()`` text, which
nadavca_amd/device.py never provokes — and the two calls it lets through without a list to walk.  One batch of 2 reads
of 40 bases (k = 6, alphabet 5, bandwidth 30, min_event_length 2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BW, MEL = 30, 2

# per entry point: its arguments behind model_wobbling in the header's order, the second level of its list as
# (total, offsets) or None, its own list arrays, and the texts of its refusals
ENTRIES = {
    'listed': dict(
        fn='nvk_estimate_hypotheses_batch_dev',
        args=('total_hyp', 'hyp_off', 'hyp_pos', 'hyp_base', 'out_total', 'out_hyp', 'out_status'),
        second=None, lists=('hyp_pos', 'hyp_base'),
        null='negative total_hyp or NULL hypothesis / output pointer',
        empty_hyp='hypothesis offsets end at 0, total_hyp is 1'),
    'joint': dict(
        fn='nvk_estimate_joint_hypotheses_batch_dev',
        args=('total_hyp', 'hyp_off', 'total_sub', 'sub_off', 'sub_pos', 'sub_base', 'out_total', 'out_hyp',
              'out_status'),
        second=('total_sub', 'sub_off'), lists=('sub_pos', 'sub_base'),
        null='negative total_hyp / total_sub or NULL hypothesis / substitution / output pointer',
        empty_hyp='hypothesis offsets end at 0, total_hyp is 1 and total_sub 0',
        empty_second='hypothesis offsets end at 0, total_hyp is 0 and total_sub 1'),
    'edit': dict(
        fn='nvk_estimate_edit_hypotheses_batch_dev',
        args=('total_hyp', 'hyp_off', 'edit_pos', 'edit_del', 'total_ins', 'ins_off', 'ins_base', 'out_total',
              'out_hyp', 'out_status'),
        second=('total_ins', 'ins_off'), lists=('edit_pos', 'edit_del', 'ins_base'),
        null='negative total_hyp / total_ins or NULL hypothesis / insertion / output pointer',
        empty_hyp='hypothesis offsets end at 0, total_hyp is 1 and total_ins 0',
        empty_second='hypothesis offsets end at 0, total_hyp is 0 and total_ins 1'),
}
TWO_LEVEL = ['joint', 'edit']


class Setup:
    """The batch on the device, every entry point's valid arguments — read 0 lists one hypothesis at position 5 (a
    substitution; for 'edit' one base deleted and one inserted), read 1 lists nothing — and the full matrix of
    nvk_estimate_log_likelihoods_batch_dev for the same reads."""

    def __init__(self):
        import torch
        from nadavca_amd import _lib, dtw, synthetic
        from nadavca_amd.device import DeviceBatch, estimate_log_likelihoods_dev
        self.lib = _lib.load()
        self.invalid, self.ok, self.read_ok = _lib.NVK_ERR_INVALID, _lib.NVK_OK, _lib.READ_OK
        model = synthetic.synth_model_arrays(41, k=6, central=2, alphabet=5)
        self.model = dtw.KmerModel(*model)
        batch = synthetic.make_batch(2, model, seed=9, R=40, R_spread=0, bandwidth=BW, dwell=(2, 9), jitter=5)
        self.dev = torch.device('cuda', self.model.context.device)
        self.db = db = DeviceBatch(batch, self.dev)
        ll, status = estimate_log_likelihoods_dev(db, BW, MEL, self.model, True)
        assert status.tolist() == [self.read_ok] * 2
        rows = torch.arange(db.total_ref, device=self.dev)
        self.ref_entries = ll[rows, db.reference.long()].cpu().numpy()   # [p, reference[p]] of every position
        self.ref_off = batch.ref_off
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=self.dev)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=self.dev)
        other = (int(batch.reference[5]) + 1) % 5
        self.tensors = dict(hyp_off=i64([0, 1, 1]), hyp_pos=i32([5]), hyp_base=i32([other]), sub_off=i64([0, 1]),
                            sub_pos=i32([5]), sub_base=i32([other]), edit_pos=i32([5]), edit_del=i32([1]),
                            ins_off=i64([0, 1]), ins_base=i32([other]), zero_off=i64([0]))
        self.totals = dict(total_hyp=1, total_sub=1, total_ins=1)

    def call(self, entry, n_reads=2, **change):
        """One call of ``entry`` with its valid arguments, except ``change`` (name -> an int, a tensor, or None for
        NULL); ``n_reads`` 0: an empty batch, NULL for its data arrays.  -> (return code, error text, out_total,
        out_hyp, out_status)."""
        import torch
        e, db = ENTRIES[entry], self.db
        out = dict(out_total=torch.full((2,), float('nan'), dtype=torch.float64, device=self.dev),
                   out_hyp=torch.full((1,), float('nan'), dtype=torch.float64, device=self.dev),
                   out_status=torch.full((2,), -9, dtype=torch.int32, device=self.dev))
        values = dict(self.totals, **self.tensors, **out)
        values.update(change)
        ptr = lambda t: None if t is None else t.data_ptr()
        if n_reads:
            head = [db.n, db.total_signal, db.total_ref, db.total_anchors] + [p.value for p in db.pointers()]
        else:
            head = [0, 0, 0, 0] + [None, ptr(self.tensors['zero_off'])] * 5
        tail = [values[a] if isinstance(values[a], int) else ptr(values[a]) for a in e['args']]
        torch.cuda.synchronize(self.dev)   # (the fills above run on torch's stream, the library on its own)
        rc = getattr(self.lib, e['fn'])(self.model.handle, *head, BW, MEL, 1, *tail)
        return (rc, self.lib.nvk_last_error().decode(), out['out_total'].cpu().numpy(), out['out_hyp'].cpu().numpy(),
                out['out_status'].cpu().numpy())

    def refused(self, entry, message, **kw):
        rc, text, total, hyp, status = self.call(entry, **kw)
        assert (rc, text) == (self.invalid, message)
        assert np.isnan(total).all() and np.isnan(hyp).all() and (status == -9).all()   # nothing was written


@pytest.fixture(scope='module')
def setup():
    return Setup()


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_negative_total_or_null_pointer(setup, entry):
    e = ENTRIES[entry]
    setup.refused(entry, e['null'], total_hyp=-1)
    for name in ('hyp_off', 'out_total', 'out_hyp') + e['lists']:   # (every total is positive)
        setup.refused(entry, e['null'], **{name: None})


@pytest.mark.parametrize('entry', TWO_LEVEL)
def test_second_level_negative_total_or_null_offsets(setup, entry):
    e = ENTRIES[entry]
    total, off = e['second']
    setup.refused(entry, e['null'], **{total: -1})
    setup.refused(entry, e['null'], **{off: None})


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_empty_batch_with_hypotheses(setup, entry):
    """n_reads == 0: the hypothesis offsets are the single 0, so a nonzero total contradicts them."""
    e = ENTRIES[entry]
    zero = setup.tensors['zero_off']
    second = {e['second'][0]: 0, e['second'][1]: zero} if e['second'] else {}
    setup.refused(entry, e['empty_hyp'], n_reads=0, hyp_off=zero, **second)
    if e['second']:
        setup.refused(entry, e['empty_second'], n_reads=0, hyp_off=zero, total_hyp=0, **{e['second'][1]: zero})


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_empty_batch_without_hypotheses(setup, entry):
    """n_reads == 0 and every total 0: NVK_OK and no device work — the lists and out_hyp may be NULL."""
    e = ENTRIES[entry]
    zero = setup.tensors['zero_off']
    change = dict(hyp_off=zero, total_hyp=0, out_hyp=None, **{name: None for name in e['lists']})
    if e['second']:
        change.update({e['second'][0]: 0, e['second'][1]: zero})
    rc, _, total, hyp, status = setup.call(entry, n_reads=0, **change)
    assert rc == setup.ok
    assert np.isnan(total).all() and np.isnan(hyp).all() and (status == -9).all()


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_read_without_hypotheses_beside_one_with(setup, entry):
    """Read 1 lists nothing, read 0 one hypothesis: NVK_OK, both reads READ_OK, and both totals are the
    reference-base entries of the full matrix, bit for bit."""
    rc, text, total, hyp, status = setup.call(entry)
    assert rc == setup.ok, text
    assert status.tolist() == [setup.read_ok] * 2
    assert not np.isnan(hyp).any()
    for j in range(2):
        want = setup.ref_entries[setup.ref_off[j]:setup.ref_off[j + 1]]
        assert not np.isnan(want).any()
        assert (want.view(np.int64) == total[j:j + 1].view(np.int64)).all()
