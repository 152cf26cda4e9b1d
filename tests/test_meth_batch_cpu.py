"""Host side of ``detect_meth_batch`` (nadavca_amd/detect_meth.py): the CSV writer of ``MethBatch`` against the
writer loop of ``detect_meth``, the contexts built from base codes, and the pattern -> codes mapping.  No GPU."""
import csv
import io

import numpy as np

from nadavca_amd.detect_meth import MethBatch, contexts_from_codes, maxs3, pattern_codes


def _detect_meth_text(rows):
    """What detect_meth's writer loop (detect_meth.py: the header, then writerow per occurrence) gives."""
    out = io.StringIO(newline='')
    writer = csv.writer(out)
    writer.writerow(('Filename', 'Position', 'Sequence context', 'Position scores', 'Aggregated score'))
    for name, pos, context, scores in rows:
        writer.writerow((name, pos, context, ','.join(map(str, scores)), maxs3(scores)))
    return out.getvalue()


def _hand_built(rng, n=40, n_reads=7):
    read = np.sort(rng.integers(0, n_reads, n)).astype(np.int64)
    position = rng.integers(5, 400, n).astype(np.int64)
    codes = rng.integers(0, 4, (n, 11))
    scores = rng.exponential(2.0, (n, 11))
    scores[0, 3] = 115.12925464970229     # -log(1e-50), the floor
    scores[1, :] = 0.0
    scores[2, 5] = 1e-17                  # repr switches to exponent notation
    scores[3, 7] = 123456789.123
    aggregate = np.array([maxs3(s.tolist()) for s in scores])
    return MethBatch(read, position, contexts_from_codes(codes), scores, aggregate,
                     np.zeros(n_reads, dtype=np.int32), np.arange(n_reads, dtype=np.int64))


def test_write_csv_equals_the_detect_meth_writer(tmp_path):
    mb = _hand_built(np.random.default_rng(5))
    rows = [('read%d' % i, int(p), str(c), s.tolist()) for i, p, c, s in zip(mb.read, mb.position, mb.context,
                                                                            mb.scores)]
    want = _detect_meth_text(rows)
    path = tmp_path / 'meth.csv'
    mb.write_csv(str(path))
    assert open(path, newline='').read() == want
    buf = io.StringIO(newline='')
    mb.write_csv(buf)
    assert buf.getvalue() == want
    names = ['r%02d.fast5' % i for i in range(7)]
    buf = io.StringIO(newline='')
    mb.write_csv(buf, names=names)
    assert buf.getvalue() == _detect_meth_text([(names[int(r[0][4:])],) + r[1:] for r in rows])


def test_write_csv_of_an_empty_batch_is_the_header():
    buf = io.StringIO(newline='')
    MethBatch.empty().write_csv(buf)
    assert buf.getvalue() == _detect_meth_text([])
    assert len(MethBatch.empty()) == 0 and MethBatch.empty().scores.shape == (0, 11)


def test_contexts_from_codes_equal_the_sequence_slices():
    rng = np.random.default_rng(6)
    seq_codes = rng.integers(0, 4, 300)
    seq = ''.join('ACGT'[c] for c in seq_codes)
    pos = np.arange(5, 295, 7)
    codes = seq_codes[pos[:, None] + np.arange(-5, 6)]
    got = contexts_from_codes(codes)
    assert got.dtype == np.dtype('U11') and got.shape == pos.shape
    assert got.tolist() == [seq[p - 5:p + 6] for p in pos]
    assert contexts_from_codes(np.zeros((0, 11), dtype=np.int64)).shape == (0,)


def test_pattern_codes():
    assert pattern_codes('CG').tolist() == [1, 2] and pattern_codes('CG').dtype == np.int32
    assert pattern_codes('ACGT').tolist() == [0, 1, 2, 3]
    assert pattern_codes('').tolist() == [] and pattern_codes('').dtype == np.int32
    assert pattern_codes('cg').tolist() == [-1, -1]
    assert pattern_codes('CCWGG').tolist() == [1, 1, -1, 2, 2]
    assert pattern_codes('N-U aé').tolist() == [-1] * 6
