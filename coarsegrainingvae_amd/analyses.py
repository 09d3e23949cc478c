"""The analyses that run after an evaluation, one record each, in the order the command-line tools run them.  ``run_ala``
(``--<stem>_eval``) and ``backmap`` (``--<stem>_stats``) take from here what they do alike for every analysis: the switch,
the ``<stem>_stats.json`` file, the ``"<stem>_stats"`` key of the summary line and its ``summary_of``.  What an analysis
asks of its own arguments stays with the tool that parses them.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

from . import contacts, coverage, density, distributions, flexibility, tica


class Analysis(NamedTuple):
    stem: str                       # --<stem>_eval, --<stem>_stats, <stem>_stats.json, "<stem>_stats"
    module: object                  # its summary_of shortens the full statistics for the summary line
    min_frames: int                 # hold-out (run_ala) or reference (backmap) frames it needs
    needs_bonds: bool
    top_level: bool                 # run_ala: at the top of the summary line, not under "test_stats"
    options: Tuple[str, ...] = ()   # run_ala: parameters that belong to the switch and are stored only with it


ANALYSES = (Analysis("dist", distributions, 2, True, True),
            Analysis("tica", tica, 2, True, True, ("tica_lag",)),
            Analysis("cov", coverage, 2, False, True),
            Analysis("contact", contacts, 2, True, False),
            Analysis("flex", flexibility, 2, True, False),
            Analysis("kde", density, 4, True, False))
BY_STEM = {a.stem: a for a in ANALYSES}
