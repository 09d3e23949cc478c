"""The host helper the step-loop trainers share (coarsegrainingvae_amd/steploop.py): the chunk loop, the checks of a frame
order table and the forced-or-rule choice of a kernel form.  No GPU."""
import numpy as np
import pytest

from coarsegrainingvae_amd import baseline, cgmap, steploop


@pytest.mark.parametrize("c", [1, 3, 8192])
def test_chunks_cover_the_steps_exactly_once_in_order(c):
    for n in (0, 1, c - 1, c, c + 1, 3 * c + 2):
        pieces = list(steploop.chunks(n, c))
        assert all(1 <= cnt <= c for _, cnt in pieces)
        assert [s for start, cnt in pieces for s in range(start, start + cnt)] == list(range(n))


def test_order_table_checks_raise_their_texts():
    good = np.array([[0, 2, 1], [1, 0, 2]], dtype=np.int64)
    assert steploop.check_order(good, 3) is good
    with pytest.raises(TypeError, match=r"^the frame order table must hold integers, not float64$"):
        steploop.check_order(good.astype(np.float64), 3)
    for empty in (np.zeros((2, 0), dtype=np.int32), np.arange(3)):
        with pytest.raises(ValueError, match=r"^order must be \[epochs, n_train\]$"):
            steploop.check_order(empty, 3)
    for bad in (good - 1, good + 1):
        with pytest.raises(ValueError, match=r"^frame order table points outside the frames$"):
            steploop.check_order(bad, 3)
    steploop.check_steps(4, 2, 2, 7, 3)                                  # two epochs of ceil(7 / 3) = 3 steps
    for first, steps in ((4, 3), (0, -1), (-1, 1)):
        with pytest.raises(ValueError, match=r"^more steps than the frame order table holds$"):
            steploop.check_steps(first, steps, 2, 7, 3)


def test_forced_form_returns_the_option_or_calls_the_rule(options):
    calls = []

    def rule():
        calls.append(1)
        return 7

    for forced in (1, 2):
        options.set("cgae_form", forced)
        assert steploop.forced_form("cgae_form", rule) == forced and not calls
    options.set("cgae_form", 0)
    assert steploop.forced_form("cgae_form", rule) == 7 and len(calls) == 1


def test_public_names_stay_where_they_were():
    assert cgmap.steps_per_epoch is steploop.steps_per_epoch and cgmap.steps_per_epoch(7, 3) == 3
    assert cgmap.CHUNK_STEPS == baseline.CHUNK_STEPS == 8192
    assert cgmap.FORM_NAMES == {cgmap.RESIDENT: "resident", cgmap.STREAMED: "streamed"}
    assert baseline.FORM_NAMES == {baseline.RESIDENT: "resident", baseline.GLOBAL: "global"}
    assert callable(cgmap.choose_form) and callable(cgmap.choose_newman_form) and callable(baseline.choose_form)
