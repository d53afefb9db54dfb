"""A gate that makes wrong-stream work visible, deterministically and without concurrency (include/sigmazero.h: "all device work is enqueued on
the caller's stream").  tests/test_gpu_stream_contract.py runs every entry point through it, tests/test_streamgate.py checks the parts below that
need no GPU.

One GATED REGION is one entry point or one short call sequence.  A test describes it once, as sess.region(name, issue, inputs, outputs, blocking),
and runs the same program under two sessions:

  Baseline   the default stream with plain synchronisation: the true inputs are copied in, the device is synchronised, issue() runs and the time the
             HOST needed to issue it is measured (time.perf_counter), the device is synchronised again and the outputs are cloned.
  Gated      a side stream S = torch.cuda.Stream() (non-blocking: nothing orders it against the default stream; independent_stream() takes one that was
             SEEN not to hold the default stream back, since streams share hardware queues):
               1. every device input buffer of the region holds POISON: a valid input of the same shape that differs from the true one on every board;
               2. on S a delay kernel of D milliseconds (torch.cuda._sleep, calibrated once per process with events; a chain of matmuls if missing),
                  D = max(10 ms, 20 x the host time the BASELINE pass measured for this region), and an event recorded right behind it;
               3. on S the true inputs are copied over the poison, device to device, from staging tensors filled and synchronised beforehand;
               4. issue() runs with S current;
               5. on S every device output is copied into a snapshot;
               6. for a region that does not block the host, the event of step 2 must still be pending now: the gate was SEEN holding while the
                  whole region was issued.  A gate that did not hold makes the test fail as inconclusive (Inconclusive), it never passes;
               7. S.synchronize() and nothing wider.
             Work that escaped to another stream runs during the delay and reads poison; a host read that synchronised another stream returns before
             the region ran.  Either shows when compare() holds the snapshots and the host values to the baseline's, bit for bit.
  misroute   the same, but issue() runs with the DEFAULT stream current while the gate stands on S: what a stream bug looks like.  It reads valid
             memory and valid inputs only, so it differs from the baseline but cannot fault.  The "teeth" tests show with it that delay, non-blocking
             stream, poison and comparison together see a misrouted launch.

Regions that block by contract ("synchronises the stream") cannot be checked with the event: they are covered by the values they return."""
import collections
import math
import os
import time

import numpy as np
import torch

MIN_DELAY_MS = 10.0
HOST_FACTOR = 20.0           # host jitter on a shared machine: the delay outlasts 20 x the measured host time of the region


class Inconclusive(AssertionError):
    """the gate was not seen holding: the run proves nothing and must not pass"""


class Diverged(AssertionError):
    """the gated pass issued another sequence of regions than its baseline"""


class Misrouted(Exception):
    """raised by a Gated session behind the region named stop_after, once a region has been misrouted: the engine's state is not the baseline's any more"""


# ---------------------------------------------------------------------------------------------------------------- delay arithmetic (CPU-checked)
def delay_ms(host_seconds):
    """D of a region whose issue took host_seconds on the baseline pass"""
    if not (host_seconds >= 0.0):
        raise ValueError("host time %r" % (host_seconds,))
    return max(MIN_DELAY_MS, HOST_FACTOR * host_seconds * 1e3)


def units_per_ms(u_lo, ms_lo, u_hi, ms_hi):
    """delay units (cycles of torch.cuda._sleep, or matmuls of the fall-back) per millisecond from two timed delays: the slope, so that the fixed
    cost of a launch drops out.  The launch cost then comes on top of every delay asked for: a gate only ever lasts longer than D."""
    if not (u_hi > u_lo > 0) or not (ms_hi > ms_lo > 0):
        raise Inconclusive("delay calibration: %r units took %r ms, %r units took %r ms" % (u_lo, ms_lo, u_hi, ms_hi))
    return (u_hi - u_lo) / (ms_hi - ms_lo)


def units_for(ms, per_ms):
    """delay units to ask for so that the delay kernel runs at least `ms`"""
    if not (ms > 0 and per_ms > 0):
        raise ValueError("units_for(%r, %r)" % (ms, per_ms))
    return int(math.ceil(ms * per_ms))


# ---------------------------------------------------------------------------------------------------------------- bookkeeping (CPU-checked)
def gate_held(event):
    """step 6: True when the event recorded behind the delay kernel has not happened yet"""
    return not event.query()


Region = collections.namedtuple("Region", "name host snaps host_seconds delay_ms held blocking misrouted")


def unheld(regions):
    """names of the gated regions whose gate was not seen holding; blocking regions (held is None) are not judged by the event"""
    return [r.name for r in regions if not r.blocking and r.delay_ms is not None and r.held is not True]


def assert_held(regions):
    bad = unheld(regions)
    if bad:
        raise Inconclusive("the gate did not hold while %d region(s) were issued (first: %s): inconclusive, not a pass" % (len(bad), bad[0]))
    return sum(1 for r in regions if not r.blocking and r.delay_ms is not None)


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        return isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def compare(base, gated):
    """the regions of a gated pass against its baseline's, raw bits: -> list of "region: what" strings, empty when everything is equal.  A misrouted
    pass stops early; the regions it issued are compared."""
    out = []
    for k, g in enumerate(gated):
        b = base[k]
        if b.name != g.name:
            out.append("region %d: baseline issued %s, the gated pass %s" % (k, b.name, g.name))
            break
        if not _same(b.host, g.host):
            out.append("%s: host values" % g.name)
        if len(b.snaps) != len(g.snaps):
            out.append("%s: %d outputs, baseline %d" % (g.name, len(g.snaps), len(b.snaps)))
            continue
        for i, (x, y) in enumerate(zip(b.snaps, g.snaps)):
            if not _same(x, y):
                out.append("%s: device output %d" % (g.name, i))
    return out


# ---------------------------------------------------------------------------------------------------------------- poison builders (CPU-checked)
def shifted(pool, n):
    """(true, poison) from a pool of n + 1 rows: the true input is rows 0..n-1, the poison the same rolled by one board (rows 1..n).  Works for one
    board too, where rolling a batch of one would change nothing."""
    assert pool.shape[0] == n + 1
    return pool[:n], pool[1:n + 1]


def policy_pool(n, rng, actions=4672):
    """n probability rows f32 (every entry positive, each row sums to 1 within f32 rounding) and n values in (-1, 1)"""
    p = rng.random((n, actions), dtype=np.float32) + np.float32(1e-3)
    p /= p.sum(axis=1, keepdims=True, dtype=np.float64).astype(np.float32)
    v = (rng.random(n, dtype=np.float32) * np.float32(1.9) - np.float32(0.95)).astype(np.float32)
    return p.astype(np.float32), v


def gate_uniforms(n, rng):
    """n uniforms in [1/64, 1/4) or (3/4, 63/64]: u and its poison 1 - u both lie in [0, 1) and are at least 1/2 apart, so sz_play's cumulative rule
    cannot choose the same child for both unless one child holds half of the visits or more (same_choice_possible)"""
    u = np.float64(1.0 / 64) + rng.random(n) * np.float64(0.25 - 1.0 / 64 - 1e-9)
    flip = rng.random(n) < 0.5
    return np.where(flip, 1.0 - u, u).astype(np.float64)


def poison_uniforms(u):
    return (1.0 - np.asarray(u, np.float64)).astype(np.float64)


def pick(visits, u):
    """np.random.choice(keys, p=visits/sum) given its uniform (sim.py:68-76 as sz_play restates it): the first child whose cumulative share exceeds u"""
    v = np.asarray(visits, np.float64)
    c = np.cumsum(v / v.sum())
    return int(min(np.searchsorted(c, u, side="right"), len(v) - 1))


def same_choice_possible(visits):
    """True when some child holds at least half of the visits: only then can u and 1 - u of gate_uniforms fall on one child"""
    v = np.asarray(visits, np.float64)
    return bool(v.max() * 2 >= v.sum())


def gate_actions(legal, rng):
    """(true, poison) int32 actions for sz_play_moves from each board's legal action list: two different legal moves; -1 for both where the game is
    over (no legal move), which the caller must not count as poisoned"""
    true, poison = [], []
    for acts in legal:
        acts = sorted(int(a) for a in acts)
        if not acts:
            true.append(-1); poison.append(-1)
            continue
        assert len(acts) >= 2, "a position with one legal move has no other legal move to poison with"
        k = int(rng.integers(len(acts)))
        true.append(acts[k]); poison.append(acts[(k + 1) % len(acts)])
    return np.array(true, np.int32), np.array(poison, np.int32)


def random_planes(n, rng, density=0.12):
    """n boards of 0/1 planes [n, 119, 8, 8] uint8, every board different from the next"""
    x = (rng.random((n, 119, 8, 8)) < density).astype(np.uint8)
    x[:, 0, 0, 0] = np.arange(n) & 1                        # neighbours differ even if the draw repeated a board
    return x


def nhwc128(planes):
    """[n,119,8,8] 0/1 -> the SZ_PLANES_NHWC128_BF16 image [n,64,128] (values 0/1, as uint8; channels 119..127 zero)"""
    n = planes.shape[0]
    out = np.zeros((n, 64, 128), np.uint8)
    out[:, :, :119] = planes.reshape(n, 119, 64).transpose(0, 2, 1)
    return out


def pack_bits128(img):
    """[n,64,128] 0/1 -> the SZ_PLANES_NHWC128_BITS image [n,1024] uint8: lane l = psub*16 + cq, byte q of its 16 bytes holds channels cq*8..cq*8+7
    (bit k = channel cq*8+k) of position q*4 + psub"""
    n = img.shape[0]
    v = img.astype(np.uint8).reshape(n, 16, 4, 16, 8)                     # [q][psub][cq][k]
    v = v.transpose(0, 2, 3, 1, 4)                                     # [psub][cq][q][k]
    return (v << np.arange(8, dtype=np.uint8)).sum(axis=-1).astype(np.uint8).reshape(n, 1024)


# ---------------------------------------------------------------------------------------------------------------- the delay kernel
class Calibration:
    """units per millisecond of the delay kernel on the current device, measured once with events on the default stream"""

    def __init__(self):
        self.kind = "torch.cuda._sleep" if hasattr(torch.cuda, "_sleep") else "matmul chain"
        if self.kind != "torch.cuda._sleep":
            self._a = torch.randn(2048, 2048, device="cuda")
        lo, hi = (2_000_000, 20_000_000) if self.kind == "torch.cuda._sleep" else (4, 40)
        self._run(lo)                                                   # first use: module load
        self.points = [(u, self._time(u)) for u in (lo, hi)]
        self.per_ms = units_per_ms(self.points[0][0], self.points[0][1], self.points[1][0], self.points[1][1])
        self.check_asked = MIN_DELAY_MS
        self.check_ms = self._time(units_for(MIN_DELAY_MS, self.per_ms))
        if self.check_ms < 0.9 * MIN_DELAY_MS:
            raise Inconclusive("delay calibration: asked for %.1f ms, the delay kernel ran %.2f ms" % (MIN_DELAY_MS, self.check_ms))

    def _run(self, units):
        if self.kind == "torch.cuda._sleep":
            torch.cuda._sleep(int(units))
        else:
            x = self._a
            for _ in range(int(units)):
                x = torch.mm(x, self._a) * 1e-2

    def _time(self, units):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); self._run(units); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def delay(self, ms):
        """enqueue a delay of at least `ms` on the current stream"""
        self._run(units_for(ms, self.per_ms))

    def lines(self):
        return ["delay kernel: %s on %s" % (self.kind, torch.cuda.get_device_name()),
                "calibration (measured with events): %s -> %.1f units per ms; %.1f ms asked for ran %.2f ms"
                % (", ".join("%d units %.3f ms" % p for p in self.points), self.per_ms, self.check_asked, self.check_ms)]


_calibration = None


def calibration():
    global _calibration
    if _calibration is None:
        _calibration = Calibration()
    return _calibration


# ---------------------------------------------------------------------------------------------------------------- a side stream that gates nothing else
def runs_beside_default(stream):
    """True when work on the default stream completes WHILE `stream` is held by the delay kernel.  A non-blocking stream is not ordered against the
    default stream by the API, but the runtime maps streams onto a few hardware queues, in order within each: a side stream that shares the default
    stream's queue holds the default stream's work back too, and a launch that escaped to the default stream would then run behind the delay and the
    true inputs, unseen.  (Measured on the MI355X with four hardware queues per process: without this probe three of the misrouted regions of the teeth
    tests passed unseen; with it 24 of the 108 draws from torch's stream pool in one run of the test file were turned away, profiles/stream_contract.txt.)"""
    cal = calibration()
    probe = torch.zeros(64, device="cuda")
    held, free = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        cal.delay(MIN_DELAY_MS)
        held.record(stream)
    probe.add_(1.0)                                                     # on the default stream
    free.record(torch.cuda.default_stream())
    free.synchronize()                                                  # waits for the default stream's work alone
    beside = gate_held(held)
    torch.cuda.synchronize()
    return beside


_rejected = []                                                          # one entry per draw turned away


def independent_stream(tries=16):
    """a non-blocking side stream that does not hold the default stream back (runs_beside_default); Inconclusive when none is found.  torch.cuda.Stream()
    draws round-robin from a fixed pool per device, so a stream turned away comes round again and is probed and turned away again: independent_stream.log
    and _rejected count DRAWS from the pool, not distinct streams."""
    for k in range(tries):
        s = torch.cuda.Stream()
        if runs_beside_default(s):
            independent_stream.log.append(k)
            return s
        _rejected.append(k)
    raise Inconclusive("no side stream out of %d ran beside the default stream: a gate on it would hold misrouted work back too" % tries)


independent_stream.log = []


# ---------------------------------------------------------------------------------------------------------------- the two sessions
def _outputs(outputs, host):
    return list(outputs(host)) if callable(outputs) else list(outputs)


class Baseline:
    """the default stream, plain synchronisation; measures the host time of every region"""
    gated = False

    def __init__(self):
        self.regions = []
        assert torch.cuda.current_stream() == torch.cuda.default_stream(), "the baseline runs on the default stream"

    def region(self, name, issue, inputs=(), outputs=(), blocking=False):
        with torch.no_grad():
            for buf, true, _ in inputs:
                buf.copy_(true)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = issue()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        snaps = [o.detach().clone() for o in _outputs(outputs, host)]
        torch.cuda.synchronize()
        self.regions.append(Region(name, host, snaps, dt, None, None, blocking, False))
        return host


class Gated:
    """the same program behind a gate on a side stream.  baseline: the Baseline session of the same program (its host times size the delays, its
    region names guard the sequence).  misroute: name of the region to issue on the default stream; stop_after: the region behind which Misrouted is
    raised (default: the misrouted one).  Every region is gated."""
    gated = True

    def __init__(self, baseline, stream=None, misroute=None, stop_after=None):
        self.base = baseline.regions
        self.stream = stream if stream is not None else independent_stream()
        self.cal = calibration()
        self.misroute, self.stop_after = misroute, stop_after or misroute
        self.regions = []
        self._misrouted = False

    def region(self, name, issue, inputs=(), outputs=(), blocking=False):
        k = len(self.regions)
        if k >= len(self.base) or self.base[k].name != name:
            raise Diverged("region %d: the gated pass issues %s, the baseline issued %s" % (k, name, self.base[k].name if k < len(self.base) else "nothing more"))
        ref = self.base[k]
        D = delay_ms(ref.host_seconds)
        mis = name == self.misroute and not self._misrouted
        S = self.stream
        with torch.no_grad():
            for buf, true, poison in inputs:                            # step 1, on the default stream, finished before the gate goes up
                buf.copy_(poison)
        fixed = None if callable(outputs) else [torch.empty_like(o.detach()) for o in outputs]
        event = torch.cuda.Event()
        torch.cuda.synchronize()
        held = None
        with torch.cuda.stream(S):
            self.cal.delay(D)                                           # step 2
            event.record(S)
            with torch.no_grad():
                for buf, true, _ in inputs:                             # step 3
                    buf.copy_(true, non_blocking=True)
            if mis:                                                     # step 4
                with torch.cuda.stream(torch.cuda.default_stream()):
                    host = issue()
            else:
                host = issue()
            if fixed is None:                                           # step 5
                snaps = [o.detach().clone() for o in _outputs(outputs, host)]
            else:
                for s, o in zip(fixed, outputs):
                    s.copy_(o.detach(), non_blocking=True)
                snaps = fixed
            if not blocking:                                            # step 6
                held = gate_held(event)
        S.synchronize()                                                 # step 7
        self.regions.append(Region(name, host, snaps, ref.host_seconds, D, held, blocking, mis))
        if mis:
            self._misrouted = True
        if self._misrouted and name == self.stop_after:
            torch.cuda.synchronize()                                    # the misrouted work ran on the default stream
            raise Misrouted(name)
        return host


def run_pair(program, misroute=None, stop_after=None, stream=None):
    """program(sess) under a Baseline and then under a Gated session -> (baseline regions, gated regions).  program builds a FRESH engine or network
    from the same seeds each time it is called."""
    base = Baseline()
    program(base)
    torch.cuda.synchronize()
    gated = Gated(base, stream=stream, misroute=misroute, stop_after=stop_after)
    try:
        program(gated)
    except Misrouted:
        pass
    torch.cuda.synchronize()
    return base.regions, gated.regions


# ---------------------------------------------------------------------------------------------------------------- the written record
def report_lines(family, regions):
    """per region name of a family: how many regions, how many gated and seen holding, the measured host issue times and the delays used"""
    groups = collections.OrderedDict()
    for r in regions:
        key = r.name.split("#")[0]                                      # "step#3/1" -> "step"
        groups.setdefault(key, []).append(r)
    out = []
    for key, rs in groups.items():
        ht = [r.host_seconds * 1e3 for r in rs]
        ds = [r.delay_ms for r in rs if r.delay_ms is not None]
        nb = [r for r in rs if not r.blocking and r.delay_ms is not None]
        out.append("%-28s %-26s n=%-4d host issue %.3f..%.3f ms  D %s ms  %s" % (
            family, key, len(rs), min(ht), max(ht), "%.1f..%.1f" % (min(ds), max(ds)) if ds else "-",
            "blocking: judged by its values" if not nb else "held %d/%d" % (sum(1 for r in nb if r.held), len(nb))))
    return out


def write_report(family, regions):
    """append a family's lines to the file named by SZ_STREAM_CONTRACT_REPORT (profiles/stream_contract.txt is such a file); without the variable the
    lines are printed only"""
    lines = report_lines(family, regions)
    path = os.environ.get("SZ_STREAM_CONTRACT_REPORT")
    if path:
        new = not os.path.exists(path) or getattr(write_report, "_pid", None) != os.getpid()
        with open(path, "w" if new else "a") as f:
            if new:
                f.write("\n".join(["# the stream contract's gate (tests/streamgate.py): D = max(%.0f ms, %.0f x host issue time of the region on the default-stream pass)"
                                   % (MIN_DELAY_MS, HOST_FACTOR)] + calibration().lines()) + "\n")
                write_report._pid = os.getpid()
            f.write("\n".join(lines) + "\n")
            f.write("%-28s side-stream draws from torch's pool so far: %d taken, %d turned away because they held the default stream back\n" % (family, len(independent_stream.log), len(_rejected)))
    print("\n".join(lines))
    return lines
