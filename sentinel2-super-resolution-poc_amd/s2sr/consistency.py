"""Host-side helpers of the radiometric consistency pass: the mode names and the refusals every layer above the
engine shares.  The device work -- one back-projection step on the quantised image, behind the paste -- is in csrc/consistency.hip,
behind native.Engine.enhance_consistent_* and native.Engine.consistency."""
from __future__ import annotations

from typing import Optional

EXACT, SMOOTH = 1, 2                       # S2SR_CONSISTENCY_*
MODES = {"exact": EXACT, "smooth": SMOOTH}
NAMES = {v: k for k, v in MODES.items()}


def mode_of(consistency) -> int:
    """None -> 0 (off), "exact" -> 1, "smooth" -> 2; anything else is a ValueError (before anything is created)."""
    if consistency is None:
        return 0
    if isinstance(consistency, str) and consistency in MODES:
        return MODES[consistency]
    raise ValueError(f"consistency {consistency!r}: None, \"exact\" or \"smooth\"")


def check_args(consistency, what: str = "consistency") -> Optional[str]:
    """The refusal alone; returns the name (or None)."""
    try:
        mode_of(consistency)
    except ValueError as e:
        raise ValueError(str(e).replace("consistency", what, 1)) from None
    return consistency


def metadata_block(consistency, inexact, applied_before: Optional[str] = None) -> dict:
    """The "consistency" block of a job's metadata: the mode, the inexact blocks per band (R, G, B) and, where a post-process
    follows the pass, that the product was consistent before it."""
    block = {"mode": check_args(consistency), "inexact_blocks": [int(v) for v in inexact]}
    if applied_before:
        block["applied_before"] = applied_before
    return block
