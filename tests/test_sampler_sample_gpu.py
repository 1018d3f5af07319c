"""GPU: Sampler*.sample() of every sampler equals the one-unit problem it stands for, written out here by hand -- the numeric
sampler id and the explicit parameter keys, nothing taken from the registry -- under the same seed.

The input is the smallest that reaches every branch of sample(): one contig, a workspace of six pieces of 50 bases, 100
apart, and three segments that are whole pieces of it.  SamplerUniverse then draws k = 3 of m = 6 pieces, SamplerLocalPermutation
has short segments well inside [0, piece end), SamplerBruteForce can add its overlaps up exactly."""
import random

import numpy as np
import pytest

import gat_amd
from gat_amd import _lib
from gat_amd import intervals as iv

pytestmark = pytest.mark.gpu

WORKSPACE = [(100 + 100 * i, 150 + 100 * i) for i in range(6)]
SEGMENTS = [WORKSPACE[0], WORKSPACE[2], WORKSPACE[5]]

# class, its parameters, a seed, and the keys the one-unit problem of sample() carries for it
CASES = [
    (gat_amd.SamplerAnnotator, dict(bucket_size=2, nbuckets=5000), 11, dict(bucket_size=2, nbuckets=5000)),
    (gat_amd.SamplerSegments, dict(bucket_size=1, nbuckets=3000), 12, dict(bucket_size=1, nbuckets=3000, sampler=1)),
    (gat_amd.SamplerShift, dict(radius=3.5, extension=40), 13, dict(sampler=2, shift_radius=3.5, shift_extension=40)),
    (gat_amd.SamplerGlobalPermutation, {}, 14, dict(sampler=3)),
    (gat_amd.SamplerLocalPermutation, {}, 15, dict(sampler=4)),
    (gat_amd.SamplerBruteForce, dict(bucket_size=1, nbuckets=4000, ntries_inner=90, ntries_outer=9), 16,
     dict(bucket_size=1, nbuckets=4000, sampler=5, brute_ntries_inner=90, brute_ntries_outer=9)),
    (gat_amd.SamplerCircular, {}, 17, dict(sampler=6)),
    (gat_amd.SamplerUniverse, {}, 18, dict(sampler=7)),
]


@pytest.fixture(scope="module")
def ctx():
    return gat_amd.get_context()


@pytest.mark.parametrize("cls,params,seed,keys", CASES, ids=[c[0].__name__ for c in CASES])
def test_sample_is_the_one_unit_problem(ctx, cls, params, seed, keys):
    segments = gat_amd.SegmentList(iter=SEGMENTS, normalize=True)
    workspace = gat_amd.SegmentList(iter=WORKSPACE, normalize=True)
    s, w = iv.make([a for a, _ in SEGMENTS], [b for _, b in SEGMENTS]), iv.make([a for a, _ in WORKSPACE], [b for _, b in WORKSPACE])
    assert np.array_equal(segments.asArray(), s) and np.array_equal(workspace.asArray(), w)
    flat = dict(n_units=1, segs=s, seg_off=[0, len(s)], ws=w, ws_off=[0, len(w)], unit_contig=[0], n_contigs=1,
                merge_contigs=0, n_tracks=0, annos=iv.EMPTY, anno_off=[0], cws_nseg=[len(w)], **keys)
    P = _lib.Problem(ctx, flat)
    try:
        seg, off = P.sample(seed, 0, 1)
        stats = P.last_stats
    finally:
        P.close()
    want = seg[off[0]:off[1]]
    sampler = cls(**params)
    got = sampler.sample(segments, workspace, seed=seed)
    assert type(got) is gat_amd.SegmentList
    assert len(want) > 0 and np.array_equal(got.asArray(), want)
    assert bool(got.isNormalized) == (cls is not gat_amd.SamplerSegments)
    if cls is gat_amd.SamplerAnnotator:
        assert sampler.nunsuccessful_rounds == stats["n_unsuccessful"]
    # the default seed is the draw of the class's generator: numpy's, or Python's random for the two permutations
    np_saved, py_saved = np.random.get_state(), random.getstate()
    try:
        np.random.seed(seed)
        random.seed(seed)
        drawn = random.getrandbits(32) if cls in (gat_amd.SamplerGlobalPermutation, gat_amd.SamplerLocalPermutation) \
            else int(np.random.randint(0, 2 ** 32))
        np.random.seed(seed)
        random.seed(seed)
        by_default = cls(**params).sample(segments, workspace)
    finally:
        np.random.set_state(np_saved)
        random.setstate(py_saved)
    assert np.array_equal(by_default.asArray(), cls(**params).sample(segments, workspace, seed=drawn).asArray())
