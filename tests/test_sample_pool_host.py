"""Host (no GPU): the one skeleton under the five sample pools' Python counters (vocoder_amd.sample_pool.SamplePoolCounters) — every class
is one, a step that breaks several rules raises the refusal the library's order dictates (csrc/sample_pool.h sample_pool_admit: per item a
session out of range, a duplicate, samples outside [0, max_chunk], a flushed slot, 2^40) with one text from every class, a pool's own
refusal (the wav pool's too-short flush, the pitch-shift pool's 2^30) comes only after the whole first pass, and a refused plan or step
moves no counter."""
import copy

import pytest

from vocoder_amd import f0, framing, pitch_shift as ps, resample as rs
from vocoder_amd.sample_pool import MAX_SAMPLES, SamplePoolCounters
from vocoder_amd.sessions import PoolStateError

S, MAX_CHUNK = 4, 8
_shift: list = []


def _pv():
    if not _shift:
        _shift.append(ps.PitchShift(8000, 3, n_fft=64, hop_length=16))
    return ps.PvPoolCounters(_shift[0], S, MAX_CHUNK)


MAKE = {
    "wav": lambda: framing.PoolCounters(framing.Framing(32, 32, 4), S, MAX_CHUNK),
    "resample": lambda: rs.ResamplePoolCounters(rs.design(2, 3), S, MAX_CHUNK),
    "yin": lambda: f0.YinPoolCounters(64, 16, S, MAX_CHUNK),
    "osc": lambda: f0.OscPoolCounters(S, MAX_CHUNK),
    "pv": _pv,
}
# (items, the refusal, its text): each step breaks a second rule that stands later in the library's order.  Slot 2 is flushed and one sample
# short of 2^40 (_counters).
ORDER = [
    ([(1, 1, False), (9, 99, False), (1, 1, False)], ValueError, "item 1 names session 9, outside [0, 4)"),             # before item 2's duplicate
    ([(1, 1, False), (1, 99, False)], ValueError, "duplicate session 1 (item 1): a session appears at most once per step"),   # before its 99 samples
    ([(2, 99, False)], ValueError, "item 0 (session 2) has 99 samples, outside [0, max_chunk = 8]"),                      # before the flushed slot
    ([(2, 5, False)], PoolStateError, "session 2 was flushed (item 0); reset it before the next utterance"),              # before 2^40
    ([(0, 1, False), (3, 2, True)], ValueError, "item 1 takes session 3 past 2^40 samples in one utterance"),
]


def _counters(kind):
    """Counters that have moved: slots 0 and 1 hold samples, slot 2 is flushed, slots 2 and 3 stand one sample before 2^40."""
    pc = MAKE[kind]()
    pc.step([(0, 5, False), (1, 8, False)])
    pc.step([(2, 0, True), (0, 3, False)])
    pc.received[2] = pc.received[3] = MAX_SAMPLES - 1
    return pc


def _state(pc):
    return copy.deepcopy((pc.received, pc.emitted, pc.flushed))


def _refused(pc, items, error, text):
    """plan and step both raise ``error`` with exactly ``text`` and move nothing."""
    for call in (pc.plan, pc.step):
        before = _state(pc)
        with pytest.raises(error) as e:
            call(items)
        assert type(e.value) is error and str(e.value) == text, (call.__name__, str(e.value))
        assert _state(pc) == before, call.__name__


@pytest.mark.parametrize("kind", sorted(MAKE))
def test_every_counters_class_is_the_one_skeleton(kind):
    pc = _counters(kind)
    assert isinstance(pc, SamplePoolCounters)
    for name in ("plan", "commit", "step", "reset", "_items"):      # the protocol is stated once: a pool overrides only its rule
        assert name not in vars(type(pc)), name
    assert "_emission" in vars(type(pc))
    assert pc.received[:2] == [8, 8] and pc.flushed == [False, False, True, False]
    assert pc.step([]) == []
    pc.reset(2)
    assert (pc.received[2], pc.emitted[2], pc.flushed[2]) == (0, 0, False)


@pytest.mark.parametrize("kind", sorted(MAKE))
@pytest.mark.parametrize("items,error,text", ORDER)
def test_a_step_that_breaks_several_rules_raises_the_first_in_the_librarys_order(kind, items, error, text):
    _refused(_counters(kind), items, error, text)


def test_the_shared_refusals_have_one_text_in_every_class():
    for items, error, _ in ORDER:
        texts = set()
        for kind in MAKE:
            with pytest.raises(error) as e:
                _counters(kind).plan(items)
            texts.add(str(e.value))
        assert len(texts) == 1, texts


@pytest.mark.parametrize("kind,trip,text", [
    ("wav", lambda pc: (0, 0, True), "session 0 (item 0) ends after 8 samples: too short for reflect padding 14/14 and one 32-sample frame"),
    ("pv", lambda pc: pc.received.__setitem__(0, ps.MAX_UTTERANCE - 1) or (0, 5, False),
     "item 0 takes session 0 past 2^30 samples in one utterance"),
])
def test_a_pools_own_refusal_waits_for_the_whole_first_pass(kind, trip, text):
    """Item 0 trips the pool's own rule and item 1 a shared one: the shared one is raised, as sample_pool_admit runs over all items before
    the pool's rule sees any.  Alone, item 0 gets the pool's own text."""
    pc = _counters(kind)
    first = trip(pc)
    _refused(pc, [first, (1, 99, False)], ValueError, "item 1 (session 1) has 99 samples, outside [0, max_chunk = 8]")
    _refused(pc, [first, (2, 1, False)], PoolStateError, "session 2 was flushed (item 1); reset it before the next utterance")
    _refused(pc, [first, (1, 1, False)], ValueError, text)
    _refused(pc, [(1, 1, False), first], ValueError, text.replace("item 0", "item 1"))
