"""Engines for the GPU tests: the one place that knows which S2SR_* environment switches a handle reads.

s2sr_create reads every switch ONCE.  So a cached default-configuration engine is created with the switches cleared, whatever a
test has put into the environment (a cached handle never carries a test's setting), and a test of a switch creates its own
handle after setting it (fresh) and checks that the handle took it (s2sr_debug_get_config).
tests/test_abi_cpu.py holds SWITCHES to the getenv calls of s2sr_create."""
import contextlib
import os

from s2sr import native
from s2sr import weights as W

# exactly the names s2sr_create (csrc/engine.hip) reads
SWITCHES = ("S2SR_GRAPH", "S2SR_MOSAIC", "S2SR_SMALL8", "S2SR_F16_FULL", "S2SR_LAST_FOLD", "S2SR_D2H_STAGED", "S2SR_FP8_TAIL",
            "S2SR_LO_EXP", "S2SR_FP8_XEXP", "S2SR_FP8_GEXP")

_DEFAULT = {}


def state_dict(num_block, scale=4, arch="rrdb", **sd_kw):
    """The seeded (seed 0) weights of the architecture."""
    if arch == "compact":
        return W.synthetic_compact_state_dict(num_block, seed=0, **sd_kw)
    return W.synthetic_state_dict(num_block, seed=0, scale=scale, **sd_kw)


def default(num_block, precision, scale=4, arch="rrdb", **sd_kw):
    """Cached default-configuration engine with the seeded weights loaded (sd_kw: keyword arguments of the state dict)."""
    key = (num_block, precision, scale, arch, tuple(sorted(sd_kw.items())))
    if key not in _DEFAULT:
        saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        try:
            e = native.Engine(num_block=num_block, precision=precision, scale=scale, arch=arch)
        finally:
            os.environ.update(saved)
        e.load_state_dict(state_dict(num_block, scale, arch, **sd_kw))
        _DEFAULT[key] = e
    return _DEFAULT[key]


def close_default(arch):
    """Close and forget the cached engines of one architecture (a module that is done with them)."""
    for key in [k for k in _DEFAULT if k[3] == arch]:
        _DEFAULT.pop(key).close()


def fresh(monkeypatch, env, num_block, precision, scale=4, arch="rrdb", group=0, sd=None, **sd_kw):
    """A handle of its own, created with exactly the switches of `env` set; the caller closes it.  sd: the weights to load
    (default: the seeded ones, with sd_kw)."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = native.Engine(num_block=num_block, precision=precision, group=group, scale=scale, arch=arch)
    e.load_state_dict(sd if sd is not None else state_dict(num_block, scale, arch, **sd_kw))
    return e


@contextlib.contextmanager
def bare(num_block=1, **kw):
    """An engine without weights, for the passes that need none (kw: precision=...), made with every diagnostic mode off and closed
    at the end.  (diag imports this module, so it is imported here.)"""
    import diag
    with diag.modes_off():
        e = native.Engine(num_block=num_block, **kw)
        try:
            yield e
        finally:
            e.close()
