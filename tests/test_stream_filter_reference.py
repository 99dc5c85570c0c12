"""The numpy reference of a filter stream's commit (tests/stream_filter_reference.py) against the one-call
backtrack of tests/smc_reference.py: however an ancestor table is cut into chunks, the frames committed on the way followed
by the pending lineage of any final particle are that particle's path through the whole table."""
import numpy as np
import pytest

import smc_reference as SR
import stream_filter_reference as SF


def _path(anc, hist, P, m, p):
    """smc_reference.backtrack's path of final particle p of melody m: weights that put everything on p"""
    G = anc.shape[1] // P
    logW = np.full((G, P), -np.inf)
    logW[:, p] = 0.0
    with np.errstate(divide='ignore'):
        out, picks = SR.backtrack(logW, anc, hist, 1, seed=3, step=99)
    assert np.all(picks == p)
    return out[m, 0]


SEEN = dict(nothing=False, everything=False, differ=False)


@pytest.mark.parametrize("P", SF.PARTICLES)
@pytest.mark.parametrize("chunks", SF.CHUNKINGS, ids=lambda c: "x".join(map(str, c)))
def test_commits_then_any_final_lineage_is_the_backtrack(P, chunks):
    anc, hist = SF.table(P)
    assert sum(chunks) == SF.STEPS == anc.shape[0]
    pend = SF.Pending(SF.G, P, hist.shape[2])
    emitted = [[] for _ in range(SF.G)]
    k = 0
    for n in chunks:
        before = pend.pending()
        counts, frames = pend.feed(anc[k:k + n], hist[k:k + n])
        k += n
        assert np.array_equal(pend.pending(), before + n - counts)
        SEEN['nothing'] |= bool((counts == 0).any())
        SEEN['everything'] |= bool((counts == before + n).any())
        SEEN['differ'] |= len(set(counts.tolist())) > 1
        for m in range(SF.G):
            assert frames[m].shape == (counts[m], hist.shape[2])
            emitted[m].append(frames[m])
    assert np.array_equal(SF.schedule(anc, P, chunks).sum(0) + pend.pending(), np.full(SF.G, SF.STEPS))
    for m in range(SF.G):
        head = np.concatenate(emitted[m])
        for p in range(P):
            got = np.concatenate([head, SF.lineage_frames(pend.anc[m], pend.hist[m], p)])
            assert np.array_equal(got, _path(anc, hist, P, m, p)), (m, p)


def test_the_tables_cover_the_three_outcomes():
    """over the tables above: a melody that commits nothing in some chunk, one that commits everything it holds, and two
    melodies with different counts in one chunk (runs after the parametrised test: pytest keeps a file's order)"""
    if not any(SEEN.values()):              # run alone: walk the tables here
        for P in SF.PARTICLES:
            for chunks in SF.CHUNKINGS:
                test_commits_then_any_final_lineage_is_the_backtrack(P, chunks)
    assert all(SEEN.values()), SEEN


def test_commit_of_a_single_step():
    # two particles swap: nothing final; both onto particle 1: final, and the frame is particle 1's
    hist = np.arange(2 * 3, dtype=np.uint8).reshape(1, 2, 3)
    n, f, (ra, rh) = SF.commit(np.array([[1, 0]]), hist)
    assert n == 0 and f.shape == (0, 3) and ra.shape == (1, 2) and rh.shape == (1, 2, 3)
    n, f, (ra, rh) = SF.commit(np.array([[1, 1]]), hist)
    assert n == 1 and np.array_equal(f[0], hist[0, 1]) and ra.shape == (0, 2)
    # a later step that funnels everything through one particle makes the earlier step final too
    n, f, _ = SF.commit(np.array([[1, 0], [0, 0]]), np.concatenate([hist, hist + 10]))
    assert n == 2 and np.array_equal(f[0], hist[0, 1]) and np.array_equal(f[1], hist[0, 0] + 10)


def test_collapse_pick_follows_the_weights_and_its_own_stream():
    from oracle import philox as OP
    P = 5
    for want in range(P):                   # all the weight on one particle: that one, whatever the uniform
        lw = np.full(P, -np.inf)
        lw[want] = 0.0
        with np.errstate(divide='ignore'):
            assert SF.collapse_pick(lw, seed=7, t=3, m0=2) == want
    lw = np.full(P, -np.log(P))
    picks = {SF.collapse_pick(lw, seed=7, t=t, m0=0) for t in range(40)}
    assert len(picks) > 1
    u = OP.uniform(1, 7, step=3, stream_id=SF.COLLAPSE_STREAM, first_index=2)[0]
    assert SF.collapse_pick(lw, seed=7, t=3, m0=2) == min(int(np.float64(u) * P), P - 1)
    assert SF.COLLAPSE_STREAM != SR.SMC_STREAM
