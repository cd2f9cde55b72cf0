"""ops.history_span, the one range rule of the readers of a stream's history (StreamGroups.draw, motion, field, objects), against a
brute-force restatement: the set of frames a call reads is written out and the verdict is taken from that set.  No GPU, no tensors."""
import itertools

from cotracker_amd.ops import history_span


def frames_read(f0, F, back, fwd, to):
    """Every frame a call for [f0, f0 + F) reads: the frames themselves and, for each, the `back` frames before it, the frame `fwd`
    after it and the fixed frame `to`; a source below frame 0 does not exist and is dropped."""
    read = set()
    for f in range(f0, f0 + F):
        sources = [f - k for k in range(1, back + 1)]
        if fwd:
            sources.append(f + fwd)
        if to >= 0:
            sources.append(to)
        read |= {f} | {s for s in sources if s >= 0}
    return read


def verdict(committed, T_cap, ring, f0, F, back, fwd, to):
    read = frames_read(f0, F, back, fwd, to)
    if f0 < 0 or F < 1 or any(f >= committed for f in read):
        return "beyond"
    oldest = max(committed - T_cap, 0) if ring else 0
    if any(f < oldest for f in read):
        return "left"
    if max(max(read) - min(read) + 1, F + back + fwd) > T_cap:
        return "span"
    return None


def kind(answer):
    return None if answer is None else answer[0]


def test_every_case_of_the_sweep_agrees_with_the_frames_that_are_read():
    seen = {None: 0, "beyond": 0, "left": 0, "span": 0}
    for committed, T_cap, ring in itertools.product((1, 5, 12, 40), (8, 12), (False, True)):
        if not ring and T_cap < committed:
            T_cap = committed  # (a linear history holds every committed frame; the pair with the smaller cap becomes this one again)
        for f0, F, back, fwd, to in itertools.product(range(-1, committed + 1), (0, 1, 3, T_cap), (0, 1, 3, T_cap), (0, 2),
                                                      (-1, 0, committed - 1, committed)):
            if back > 0 and fwd > 0:
                continue  # (no reader looks both ways: a lag is positive or negative)
            want = verdict(committed, T_cap, ring, f0, F, back, fwd, to)
            got = history_span(committed, T_cap, ring, f0, F, back=back, fwd=fwd, to=to)
            assert kind(got) == want, (committed, T_cap, ring, f0, F, back, fwd, to, got)
            if got is not None and f0 >= 0 and F >= 1 and f0 + F <= committed:  # the range it names is the range that is read
                read = frames_read(f0, F, back, fwd, to)
                assert got[1:] == (min(read), max(read))
            seen[want] += 1
    assert all(n > 100 for n in seen.values()), seen  # every answer is exercised


def test_the_cases_of_the_readers():
    """One per reader, with the numbers of the stream tests on the GPU (window 8, step 4)."""
    # draw: a linear history of 16 frames in 32 rows, all 16 pictures with a trail of 17 -- 33 rows; a ring of 32 rows 44 frames in
    # with a trail of 4: frame 16 is the oldest picture it can still draw
    assert history_span(16, 32, False, 0, 16, back=17) == ("span", 0, 15)
    assert history_span(44, 32, True, 16, 1, back=4) is None
    assert history_span(44, 32, True, 15, 1, back=4) == ("left", 11, 15)
    # motion: the same ring, lag 1
    assert history_span(44, 32, True, 13, 2, back=1) is None
    assert history_span(44, 32, True, 12, 2, back=1) == ("left", 11, 13)
    assert history_span(44, 32, True, 43, 2, back=1) == ("beyond", 43, 44)
    # field: a ring of 16 rows 44 frames in; frame 16 as the source has left it, an anchor of it has not; forward flow of the newest
    # frames needs frames not tracked yet
    assert history_span(44, 16, True, 40, 4, to=16) == ("left", 16, 43)
    assert history_span(44, 16, True, 40, 4) is None
    assert history_span(44, 16, True, 40, 4, fwd=1) == ("beyond", 40, 44)
    assert history_span(44, 16, True, 40, 2, fwd=2) is None
    # objects: a ring of 16 rows 36 frames in, frame 22 against frame 18; two frames from the newest on against an anchor
    assert history_span(36, 16, True, 22, 1, back=4) == ("left", 18, 22)
    assert history_span(36, 16, True, 35, 2) == ("beyond", 35, 36)
