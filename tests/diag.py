"""What the modules that run under a diagnostic mode share (red zones, poison, stall, grid cap; tests/test_gpu_redzones.py, _poison.py,
_stall.py, _gridcap.py, and the pass modules that run a case of their own under a mode): engines made and closed under a mode, the
door table's baseline with every mode off, the two comparisons -- byte for byte against the baseline (same), sample for sample against
a model with the first differing position (same_values) --, the red-zone verdict, and the grid cap in force with its counter
(under, trips)."""
import contextlib

import numpy as np

import gpu_engines
from doors import CONFIGS, DOORS, Inputs
from s2sr import native

Z = 65536                        # the red-zone size of every module that runs under zones


def new_engine(name):
    """a fresh engine of CONFIGS[name] with the seeded weights, allocated under whatever modes are in force"""
    nb, prec, scale, arch = CONFIGS[name]
    e = native.Engine(num_block=nb, precision=prec, scale=scale, arch=arch)
    e.load_state_dict(gpu_engines.state_dict(nb, scale, arch))
    return e


@contextlib.contextmanager
def engines_under(read, write, value=None):
    """One mode's engines: read() / write(v) are the mode's getter and setter (native.redzone_bytes / native.redzone,
    native.poison_pattern / native.poison).  Yields get(name, v=value) -> the engine of that config created, and its weights
    loaded, with write(v) in force; each is made once.  A `value` given here is in force from the start.  At the end all are
    closed and the mode is put back to what was found (off, or what the environment set for the whole run)."""
    before = read()
    if value is not None:
        write(value)
    made = {}

    def get(name, v=value):
        if (name, v) not in made:
            write(v)
            made[name, v] = new_engine(name)
        return made[name, v]
    try:
        yield get
    finally:
        for e in made.values():
            e.close()
        write(before)


@contextlib.contextmanager
def modes_off():
    """all four modes off, each put back afterwards: what runs inside allocates, reads, waits and deals its work out as the shipped
    library does"""
    zone, pattern, (mode, usec), cap = native.redzone_bytes(), native.poison_pattern(), native.delay_mode(), native.grid_cap_workgroups()
    native.redzone(0), native.poison(0), native.delay(0), native.grid_cap(0)
    try:
        yield
    finally:
        native.redzone(zone), native.poison(pattern), native.delay(mode, usec), native.grid_cap(cap)


def keep(r):
    """results may live in the pinned pool, which the next call reuses"""
    return tuple(np.array(a) for a in r) if isinstance(r, tuple) else np.array(r)


_BASELINE = {}


def baseline(ident):
    """The door on the cached engine of gpu_engines.py with the modes off: computed once per process, shared by every module and
    state that judges the door."""
    if ident not in _BASELINE:
        name, fn = DOORS[ident]
        with modes_off():
            _BASELINE[ident] = keep(fn(gpu_engines.default(*CONFIGS[name]), Inputs()))
    return _BASELINE[ident]


def same(got, want, what):
    """byte for byte, dtype and shape included"""
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: output {k} is {g.dtype} {g.shape}, the baseline {w.dtype} {w.shape}"
        differ = int((g.view(np.uint8) != w.view(np.uint8)).sum())
        assert differ == 0, f"{what}: {differ} of {g.nbytes} bytes of output {k} differ from the baseline"


def same_values(got, want, what):
    """sample for sample, dtype and shape included, against a model or another call; the message has the first differing position.
    Tuples go member by member; a member for which `want` holds None has no model and is not judged."""
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), what
        for k, (g, w) in enumerate(zip(got, want)):
            if w is not None:
                same_values(g, w, f"{what}, output {k}")
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, the first at {tuple(bad[0])}: {got[tuple(bad[0])]} against {want[tuple(bad[0])]}"


@contextlib.contextmanager
def under(cap):
    """the grid cap in force and its counter at zero; afterwards the cap that was found"""
    before = native.grid_cap_workgroups()
    native.grid_cap(cap)
    native.grid_cap_stats(reset=True)
    try:
        yield
    finally:
        native.grid_cap(before)


def trips(*families):
    """the largest trip count the grid-cap counter holds among these families (all: no argument), and the stats for the message"""
    st = native.grid_cap_stats()
    return max(t for f, (_, t) in st.items() if not families or f in families), st


def clean(e, least=4, most=None):
    """No damaged zone anywhere in the process, and the engine counts a plausible number of zoned allocations of its own.  One
    created under zones with weights loaded owns the trash page, the bias pool and at least two weight buffers, so 4, and up to
    some dozens with workspace planes.  One without weights that ran a single pass owns 3.  An engine older than the mode
    (allocated without zones): 0."""
    n, bad, msg = e.redzone_check()
    assert bad == 0, msg
    assert n >= least and (most is None or n <= most), n
    return n
