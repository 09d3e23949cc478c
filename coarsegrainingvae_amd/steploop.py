"""What the step-loop trainers' host modules share (cgmap on K13, baseline on K19; kernels' side: csrc/steploop_dev.h): the
schedule arithmetic, the checks of a frame order table, the chunk loop, and "forced by option, else the rule" for a form."""
import numpy as np

from . import options


def steps_per_epoch(n_train: int, batch_size: int) -> int:
    return -(-n_train // batch_size)


def chunks(steps: int, chunk: int):
    """(start, count) of consecutive chunks of at most ``chunk`` steps: ``range(steps)`` exactly once, in order."""
    return ((start, min(chunk, steps - start)) for start in range(0, steps, chunk))


def check_order(table: np.ndarray, n_frames: int) -> np.ndarray:
    """A frame order table is integer [epochs, n_train] and names frames in ``range(n_frames)``."""
    if table.ndim != 2 or table.shape[1] == 0:
        raise ValueError("order must be [epochs, n_train]")
    if not np.issubdtype(table.dtype, np.integer):
        raise TypeError(f"the frame order table must hold integers, not {table.dtype}")
    if table.min() < 0 or table.max() >= n_frames:
        raise ValueError("frame order table points outside the frames")
    return table


def check_steps(first_step: int, steps: int, epochs: int, n_train: int, batch_size: int) -> None:
    if steps < 0 or first_step < 0 or first_step + steps > epochs * steps_per_epoch(n_train, batch_size):
        raise ValueError("more steps than the frame order table holds")


def forced_form(option_name: str, rule) -> int:
    """The form that option ``option_name`` forces (1 or 2), else what ``rule()`` returns."""
    forced = options.get(option_name)
    return forced if forced in (1, 2) else rule()
