"""What the per-site two-sample operators share (``compare_site_levels``; ``compare_site_ranks`` /
``site_rank_tests_batch``; ``compare_site_mixtures`` / ``site_mixture_tests_batch``): the base of their result classes
with the one TSV writer, the check of ``column``, ``min_coverage``, ``reach`` and ``trim``, and for the two operators
with a device part the way there from two event tables (``host_table_tests``) and from two ReadBatches whose rows stay
on the device (``resident_tests``), each with ONE copy back (``copy_back``).  Such an operator hands over its module as
``op``: ``_check``, ``_on_device``, ``_upload_and_test``, ``_comparison`` and ``_empty`` are looked up there when they
are called, so a test can put a numpy restatement in ``_upload_and_test``'s place."""
import contextlib
import os

import numpy as np


@contextlib.contextmanager
def _open(file):
    out = open(file, 'w', newline='') if isinstance(file, (str, os.PathLike)) else file
    try:
        yield out
    finally:
        if out is not file:
            out.close()


def contig_label(contig_names):
    """contig index -> what a TSV prints for it: the name where there are names, else the index."""
    return (lambda c: str(c)) if contig_names is None else (lambda c: contig_names[c])


def _site_key(contig, position, strand, ref_len):
    """One sortable integer per (contig, position, strand): contig-local positions are below ``ref_len``."""
    return (np.asarray(contig, dtype=np.int64) * max(int(ref_len), 1) + np.asarray(position, dtype=np.int64)) * 2 \
        + np.asarray(strand, dtype=np.int64)


def _same_reference(what, a, b):
    if a.ref_len != b.ref_len or a.contig_names != b.contig_names:
        raise ValueError('%s: the two batches are over different references (ref_len %d / %d, contig_names %r / %r)'
                         % (what, a.ref_len, b.ref_len, a.contig_names, b.contig_names))


class SiteTable:
    """The base of ``SiteComparison``, ``SiteRankComparison`` and ``SiteMixtureComparison``: row arrays, one row per
    tested (contig, position, strand), named by the class's ``_FIELDS``, which begin with contig, position, strand,
    ref_base (``_INTS``: those after them that a TSV prints as %d, the others as repr(float(...))); ``column``: what
    was compared; ``contig_names`` as the batches'."""

    def __init__(self, column, contig_names=None, **rows):
        for f in self._FIELDS:
            setattr(self, f, rows[f])
        self.column, self.contig_names = column, contig_names

    def __len__(self):
        return int(self.position.size)

    def write_tsv(self, file):
        """Header, then one tab-separated row per site: contig (by name where there are names), position, strand
        (+ / -), ref, then the other fields in their order (floats as ``repr`` gives them), to a path or a text file."""
        label, fields = contig_label(self.contig_names), self._FIELDS[4:]
        cells = [(getattr(self, f), f in self._INTS) for f in fields]
        with _open(file) as out:
            out.write('contig\tposition\tstrand\tref\t' + '\t'.join(fields) + '\n')
            out.writelines('%s\t%d\t%s\t%s\t%s\n'
                           % (label(int(self.contig[i])), self.position[i], '+-'[self.strand[i]],
                              'ACGT'[self.ref_base[i]],
                              '\t'.join('%d' % x[i] if as_int else repr(float(x[i])) for x, as_int in cells))
                           for i in range(len(self)))


def check_site_test(what, column, min_coverage, reach, trim=0):
    """The parameters every site test has (``trim``: of the ``*_batch`` forms): ValueError, named ``what``, for a
    value outside its range.  -> the index of ``column`` in ``SiteLevelBatch.COLUMNS``."""
    from .site_levels import SiteLevelBatch
    if int(trim) != trim or trim < 0:
        raise ValueError('%s: trim %r is not an integer >= 0' % (what, trim))
    j = SiteLevelBatch.column_index(column)
    if int(min_coverage) != min_coverage or min_coverage < 1:
        raise ValueError('%s: min_coverage %r is not an integer >= 1' % (what, min_coverage))
    if int(reach) != reach or reach < 0:
        raise ValueError('%s: reach %r is not an integer >= 0' % (what, reach))
    return j


def site_coordinates(keys, refset):
    """Keys 2 * global position + strand -> (contig int32, position, strand int8), contig-local through ``refset``, a
    ``refset.ReferenceSet``; contig 0 with None."""
    position = keys >> 1
    contig = np.zeros(position.size, dtype=np.int32)
    if refset is not None:
        c, position = refset.locate(position)
        contig = c.astype(np.int32)
    return contig, position, (keys & 1).astype(np.int8)


def copy_back(tensors):
    """Device tensors, int64 or float64, of shape (sites,) or (sites, k), to the host in ONE copy (the floats cross as
    their bits beside the integers).  -> numpy arrays of the same dtypes and shapes."""
    import torch
    from .device import to_host
    flat = to_host(torch.cat([t.reshape(-1).view(torch.int64) for t in tensors]))
    parts = np.split(flat, np.cumsum([t.numel() for t in tensors])[:-1])
    return tuple((p.view(np.float64) if t.dtype == torch.float64 else p).reshape(tuple(t.shape))
                 for t, p in zip(tensors, parts))


def upload_rows(key_a, val_a, key_b, val_b):
    """Host rows (key int64, one f64 column) of two samples -> the default context, the four as tensors on its GPU."""
    import torch
    from . import _lib
    context = _lib.default_context()
    dev = torch.device('cuda', context.device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    return context, up(key_a, np.int64), up(val_a, np.float64), up(key_b, np.int64), up(val_b, np.float64)


def host_table_tests(op, what, a, b, column, min_coverage, reach, *params):
    """The ``compare_site_*`` of ``op`` between two ``rows=True`` SiteLevelBatches: the guards, the keys and the rows of
    ``column`` of both event tables, ``op._upload_and_test``, then the tested sites' coordinates and their ``ref_base``
    from the rows of ``a`` -> ``op._comparison``."""
    if a.events is None or b.events is None:
        raise ValueError('%s: a batch carries no event table (site_levels_batch(rows=True))' % what)
    _same_reference(what, a, b)
    check_site_test(what, column, min_coverage, reach)
    params = op._check(what, *params)
    if a.events['read'].size == 0 or b.events['read'].size == 0:
        return op._empty(column, a.contig_names)
    key = lambda x: _site_key(x.events['contig'], x.events['position'], x.events['strand'], x.ref_len)
    f8 = lambda x, c: np.asarray(x.events[c], dtype=np.float64)
    value = lambda x: f8(x, 'level') - f8(x, 'expected') if column == 'resid' else f8(x, column)
    site_key, *stats = op._upload_and_test(key(a), value(a), key(b), value(b), int(min_coverage), *params)
    contig, position = np.divmod(site_key >> 1, max(a.ref_len, 1))
    rows_key = _site_key(a.contig, a.position, a.strand, a.ref_len)
    order = np.argsort(rows_key, kind='stable')
    at = np.minimum(np.searchsorted(rows_key[order], site_key), max(rows_key.size - 1, 0))
    if site_key.size and (rows_key.size == 0 or not np.array_equal(rows_key[order][at], site_key)):
        raise ValueError('%s: the event table of the first batch holds sites that its rows do not' % what)
    ref_base = a.ref_base[order][at].astype(np.int8) if site_key.size else np.zeros(0, dtype=np.int8)
    return op._comparison(column, a.contig_names, contig.astype(np.int32), position.astype(np.int64),
                          (site_key & 1).astype(np.int8), ref_base, int(reach), *stats)


def sample_rows(read_batch, aligner, kmer_model, config, renorm_rounds, trim, j):
    """The front end of ``site_levels_batch`` for one sample, keeping 16 B per base on the device: -> (key int64, one
    f64 column, the alignment stage): device tensors, None twice where nothing aligned."""
    import torch
    from .batchflow import align_batch
    from .device import expected_levels_dev, site_level_rows_dev
    res = align_batch(read_batch, config, kmer_model, renorm_rounds, aligner)
    stage = res.stage
    L = np.asarray(aligner.reference_num).size
    if stage.n_live == 0 or L == 0:
        return None, None, stage
    sa, dbatch = stage.sa, stage.dbatch
    expected = expected_levels_dev(dbatch, kmer_model, with_contexts=True)
    key, val = site_level_rows_dev(kmer_model.context, dbatch, res.events, expected, sa.ref_start.contiguous(),
                                   sa.reverse.to(torch.int32), res.status, int(trim), L)
    return key, val[:, j].contiguous(), stage


def resident_tests(op, what, read_batch_a, read_batch_b, aligner, kmer_model, config, renorm_rounds, trim, column,
                   min_coverage, reach, *params):
    """The ``site_*_tests_batch`` of ``op`` between two ReadBatches: ``sample_rows`` per sample with ``aligner`` (one
    for both, or a pair over the same reference), the stages dropped before ``op._on_device`` runs, then the tested
    sites' coordinates (through the aligner's ``ReferenceSet`` if it has one) and ``ref_base`` -> ``op._comparison``."""
    j = check_site_test(what, column, min_coverage, reach, trim)
    params = op._check(what, *params)
    from .batchflow import load_config, load_kmer_model
    from .refset import ReferenceSet
    aligner_a, aligner_b = aligner if isinstance(aligner, (tuple, list)) and len(aligner) == 2 else (aligner, aligner)
    reference_num = np.ascontiguousarray(aligner_a.reference_num, dtype=np.int32).reshape(-1)
    if aligner_b is not aligner_a and \
            not np.array_equal(reference_num, np.asarray(aligner_b.reference_num).reshape(-1)):
        raise ValueError('%s: the two aligners are over different references' % what)
    kmer_model, config = load_kmer_model(kmer_model), load_config(config)
    key_a, val_a, stage_a = sample_rows(read_batch_a, aligner_a, kmer_model, config, renorm_rounds, trim, j)
    key_b, val_b, stage = sample_rows(read_batch_b, aligner_b, kmer_model, config, renorm_rounds, trim, j)
    names = stage.contig_names()
    if stage_a.contig_names() != names:
        raise ValueError('%s: the two aligners are over different references (contig names %r / %r)'
                         % (what, stage_a.contig_names(), names))
    del stage_a
    if key_a is None or key_b is None:
        return op._empty(column, names)
    refset = stage.reference if isinstance(stage.reference, ReferenceSet) else None
    del stage
    site_key, *stats = op._on_device(kmer_model.context, key_a, val_a, key_b, val_b, int(min_coverage), *params)
    contig, position, strand = site_coordinates(site_key, refset)
    return op._comparison(column, names, contig, position.astype(np.int64), strand,
                          reference_num[site_key >> 1].astype(np.int8), int(reach), *stats)
