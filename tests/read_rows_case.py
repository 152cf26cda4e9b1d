"""One small batch of the shapes where a per-read row pass can go wrong (nadavca_amd/csrc/read_rows.h: the read view,
the lane loop, the event clamp and the second pass over long events), for the GPU tests of the four row entries
(k-mer statistics, modified-base rows, site levels, allele rows).  Host arrays only; every test compares the kernel
with the numpy restatement it already uses.

Eleven reads, not a multiple of the four waves of a block, of at most 150 bases:

    read  bases  what it is there for
    0     70     live; the events below
    1     64     status 1, between two live reads
    2     65     live
    3     0      no bases (25 samples)
    4     5      no samples: every event is empty after the clamp
    5     4      2 * TRIM > bases: nothing counts under TRIM (nor in read 4)
    6     63     live, starts before position 0
    7     66     status -3
    8     64     live
    9     150    live, runs past the end of the reference
    10    0      no bases, no samples: the last read

Every read of 63 bases or more holds events of 127, 128, 129 and 300 samples (128 is where the second pass takes
over), one with end < start, one that starts below 0 and one that ends past the read's samples."""
import numpy as np

LENGTHS = (70, 64, 65, 0, 5, 4, 63, 66, 64, 150, 0)
STATUS = (0, 1, 0, 0, 0, 0, 0, -3, 0, 0, 0)
CONTEXTS = ((6, 6), (3, 3), (0, 0), (2, 2), (1, 0), (6, 6), (0, 1), (6, 6), (2, 3), (6, 6), (0, 0))
STARTS = (10, 20, 30, 5, 40, 50, -3, 15, 0, 100, 7)
TRIM = 3
REF_LEN = 200
EVENT_LENGTHS = (127, 128, 129, 300)
ALPHA = 4                      # letters of the reference; the modified-base rows run on 5 with mod_code 4


def build(seed=5):
    rng = np.random.default_rng(seed)
    cases, sites, gammas = [], [], []
    for j, (R, (nb, na)) in enumerate(zip(LENGTHS, CONTEXTS)):
        length = rng.integers(2, 13, R)
        if R >= 63:
            length[rng.permutation(np.arange(12, R - 8))[:len(EVENT_LENGTHS)]] = EVENT_LENGTHS
        first = int(rng.integers(0, 30)) if R else 25
        bounds = first + np.concatenate([[0], np.cumsum(length)])
        N = 0 if j in (4, 10) else int(bounds[-1]) + int(rng.integers(0, 20))
        ev = np.stack([bounds[:-1], bounds[1:]], 1).astype(np.int32)
        if R >= 63:
            ev[8] = (ev[8][1], ev[8][0])                  # end < start
            ev[9] = (-5, ev[9][1])                        # start < 0: clamped to 0
            ev[R - 7] = (ev[R - 7][0], N + 40)            # end > N: clamped to N
        cases.append(dict(signal=rng.normal(0.0, 1.0, N), reference=rng.integers(0, ALPHA, R).astype(np.int32),
                          context_before=rng.integers(0, ALPHA, nb).astype(np.int32),
                          context_after=rng.integers(0, ALPHA, na).astype(np.int32),
                          approximate_alignment=np.zeros((1, 2), np.int32), events=ev))
        # modified-base sites: the first and the last base, a run of neighbours, then singles
        pos = np.array(sorted(set(p for p in [0, R - 1, 9, 10, 11, 20, 27, 41, 60, 90, 120] if 0 <= p < R)),
                       dtype=np.int32)
        sites.append(pos)
        gammas.append(rng.choice([0.0, 1.0, 0.37], pos.size))
    R = np.array(LENGTHS, dtype=np.int64)
    ref_off = np.concatenate([[0], np.cumsum(R)]).astype(np.int64)
    total = int(ref_off[-1])
    cat = lambda key, dt: np.concatenate([np.asarray(c[key]).reshape(-1) for c in cases]).astype(dt)
    return dict(n=len(LENGTHS), total=total, cases=cases, ref_off=ref_off,
                sig_off=np.concatenate([[0], np.cumsum([c['signal'].size for c in cases])]).astype(np.int64),
                signal=cat('signal', np.float64), reference=cat('reference', np.int32),
                events=cat('events', np.int32).reshape(-1, 2), status=np.array(STATUS, dtype=np.int32),
                start=np.array(STARTS, dtype=np.int64), reverse=(np.arange(len(LENGTHS)) % 2).astype(np.int32),
                expected=rng.normal(0.0, 1.0, total), ll=rng.normal(-30.0, 12.0, (total, ALPHA)),
                ref_codes=rng.integers(0, ALPHA, REF_LEN).astype(np.int32),
                site_off=np.concatenate([[0], np.cumsum([s.size for s in sites])]).astype(np.int64),
                site_pos=np.concatenate(sites), site_gamma=np.concatenate(gammas))
