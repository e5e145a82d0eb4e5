"""TEST INFRASTRUCTURE: a plain NumPy float32 reference of the per-sample spatializer chain and of the
listener mix, from raw inputs (abi.DSP_SOURCE_PARAMS, abi.DSP_STATE, samples), and seeded input
generators for the value classes the kernels of art_dsp.hip must get right.

The fp32 operation sequence is the contract (AudioSpatializer.OnAudioFilterRead's four passes; csrc/art_dsp_math.hpp
restates it), so every comparison with this module is bit for bit (assert_same_bits). Per frame and channel:

    muffle (flag bit 0)   pm = pm + am * (x - pm);  x = pm                 MuffleDSP.LowPass
    dry boost             x = x * dry_boost                                ReverbDSP
    gain                  x = x * gain[channel]                            BinauralDSP
    low pass (bit 1)      pl = pl + a * (x - pl);  x = pl                  BinauralDSP.LowPass
    else high pass        h = a * ((ph + x) - pi);  pi = x;  ph = h;  x = h   BinauralDSP.HighPass
    volume                x = x * volume

Each NumPy float32 ufunc call rounds once and nothing is fused. A source with flag bit 2 (not stereo) keeps
its data and its state. The arithmetic is vectorised over sources and channels and loops over frames.
"""
import numpy as np

from art import abi

f32 = np.float32
KINDS = ("gaussian", "tail", "nonfinite", "overflow", "zeros", "edge")
EDGE_ALPHAS = (0.0, 1.0, 1e-40, 0.5, 1.5, -0.25)
EDGE_DRY_BOOSTS = (0.0, 1.0, 1e-20)
FLT_MIN_NORMAL = f32(1.17549435e-38)


def chain(params, states, data):
    """The chain of every source over its frames. params abi.DSP_SOURCE_PARAMS [n], states abi.DSP_STATE [n],
    data float32 [n, frames * 2] (interleaved L, R); none is modified. Returns (out [n, frames * 2], final states [n])."""
    n = params.size
    assert params.dtype == abi.DSP_SOURCE_PARAMS and states.dtype == abi.DSP_STATE and states.size == n
    x_all = np.ascontiguousarray(data, f32).reshape(n, -1, 2)
    frames = x_all.shape[1]
    flags = params["flags"].astype(np.int64)
    run = ((flags & 4) == 0)[:, None]
    mf = ((flags & 1) != 0)[:, None]
    lp = ((flags & 2) != 0)[:, None]
    col = lambda name: params[name].astype(f32)[:, None]  # noqa: E731
    am, dry, a, vol = col("muffle_alpha"), col("dry_boost"), col("filter_alpha"), col("volume")
    gain = np.stack([params["gain_left"], params["gain_right"]], axis=1).astype(f32)
    sv = states.copy().view(f32).reshape(n, 4, 2)
    pm, pl, ph, pi = (sv[:, k, :].copy() for k in range(4))
    out = x_all.copy()
    with np.errstate(all="ignore"):
        for i in range(frames):
            x = x_all[:, i, :]
            m = pm + am * (x - pm)
            pm = np.where(mf, m, pm)
            x = np.where(mf, m, x)
            x = x * dry
            x = x * gain
            low = pl + a * (x - pl)
            high = a * ((ph + x) - pi)
            pl = np.where(lp, low, pl)
            ph = np.where(lp, ph, high)
            pi = np.where(lp, pi, x)
            x = np.where(lp, low, high)
            x = x * vol
            out[:, i, :] = np.where(run, x, x_all[:, i, :])
    new = np.stack([pm, pl, ph, pi], axis=1).astype(f32)
    new = np.where(run[:, :, None], new, sv)
    assert out.dtype == f32 and new.dtype == f32
    return out.reshape(n, -1), np.ascontiguousarray(new).reshape(n, 8).view(abi.DSP_STATE).reshape(n)


def ordered_sum(wet, F, T):
    """wet float32 [F * T, frames * 2] -> [F, frames * 2]: one float32 add per target in ascending t, starting
    from the first target's buffer itself (so a -0.0 survives at T = 1)."""
    wet = wet.reshape(F, T, -1)
    acc = wet[:, 0].copy()
    with np.errstate(all="ignore"):
        for t in range(1, T):
            acc = np.add(acc, wet[:, t], dtype=f32)
    return acc


def mix(params, states, dry, F, T):
    """The listener mix: source s = f * T + t runs the chain over dry[t] (float32 [T, frames * 2]) from states[s];
    a fan's T results are summed in target order. Returns (mix [F, frames * 2], final states [F * T])."""
    d = np.ascontiguousarray(dry, f32).reshape(T, -1)
    wet, new = chain(params, states, np.tile(d, (F, 1)))
    return ordered_sum(wet, F, T), new


def _where(idx, is_state):
    s, k = int(idx[0]), int(idx[1])
    if is_state:
        return f"source {s}, state word {abi.DSP_STATE.names[k // 2]} channel {k % 2}"
    return f"source {s}, frame {k // 2}, channel {k % 2}"


def assert_same_bits(got, want, what):
    """got and want hold float32 values per source: samples [n, frames * 2] or abi.DSP_STATE [n]. NaN positions must
    be equal (payload and sign are free: host and device default NaNs differ in sign); every other element must be
    byte-equal, +0 and -0 distinguished. Reports the first differing source, frame and channel."""
    is_state = np.asarray(want).dtype == abi.DSP_STATE
    w = np.ascontiguousarray(want).view(f32)
    w = w.reshape(-1, 8) if is_state else w.reshape(w.shape[0], -1) if w.ndim > 1 else w.reshape(1, -1)
    g = np.ascontiguousarray(got).view(f32).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} values, expected {w.size}"
    g = g.reshape(w.shape)
    gn, wn = np.isnan(g), np.isnan(w)
    bad = (gn != wn) | (~wn & (g.view(np.uint32) != w.view(np.uint32)))
    if bad.any():
        idx = np.argwhere(bad)[0]
        gv, wv = g[tuple(idx)], w[tuple(idx)]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {_where(idx, is_state)}: "
                             f"got {gv!r} (0x{int(gv.view(np.uint32)):08x}), want {wv!r} (0x{int(wv.view(np.uint32)):08x})")


class Guarded:
    """A device copy of `a` between canaries: `before` bytes of 0xC3 (a sub-view: ptr is the allocation plus
    `before`), the payload, `after` bytes of 0xC3. read() checks both canaries and returns the payload's bytes."""

    def __init__(self, a, after, before=0):
        import torch
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.before, self.size, self.after = before, raw.size, after
        host = np.concatenate([np.full(before, 0xC3, np.uint8), raw, np.full(after, 0xC3, np.uint8)])
        self.t = torch.from_numpy(host).to(torch.device("cuda", 0))
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + before

    def write(self, a):
        import torch
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert raw.size == self.size
        self.t[self.before:self.before + self.size] = torch.from_numpy(raw.copy()).to(self.t.device)

    def read(self, what):
        h = self.t.cpu().numpy()
        assert (h[:self.before] == 0xC3).all(), f"{what}: bytes before the buffer were written"
        assert (h[self.before + self.size:] == 0xC3).all(), f"{what}: bytes after the buffer were written"
        return h[self.before:self.before + self.size].copy()


# ---------------------------------------------------------------------------- inputs
def class_sources(rng, classes, frames, volume=(0.0, 2.0)):
    """One stereo art.dsp.AudioSource per entry of `classes` with random per-buffer inputs whose parameters land in
    that filter class (flags & 3: bit 0 muffle on, bit 1 low pass); an entry of 4 gives a mono source (flag bit 2)."""
    from art.dsp import AudioSource
    out = []
    for c in classes:
        d = rng.standard_normal(3)
        d[1] = -abs(d[1]) - 0.05 if c & 2 else abs(d[1]) + 0.05
        d /= np.linalg.norm(d)
        out.append(AudioSource(data=np.zeros(frames * (1 if c == 4 else 2), f32), channels=1 if c == 4 else 2,
                               muffle_strength=float(rng.uniform(0.1, 1.0)) if c & 1 else 0.0,
                               reverb_volume=float(rng.random()), local_dir=tuple(float(v) for v in d),
                               listener_distance=float(rng.uniform(0, 30)), volume_multiplier=float(rng.uniform(*volume))))
    return out


def class_params(rng, classes, settings=None, sample_rate=48000):
    """abi.DSP_SOURCE_PARAMS of class_sources, as art_dsp_source_params_get derives them (default settings)."""
    import art
    from art.dsp import SpatializerSettings
    st = settings or SpatializerSettings()
    p = np.concatenate([art.dsp.source_params(st, s, sample_rate) for s in class_sources(rng, classes, 1)])
    got = np.where(p["flags"] & 4, 4, p["flags"] & 3)
    assert (got == np.asarray(classes)).all(), (got, classes)
    return p


def log_uniform(rng, lo, hi, shape):
    """Magnitudes log-uniform in [lo, hi] with a random sign, float32."""
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), shape)) * rng.choice([-1.0, 1.0], shape)
    return v.astype(f32)


def _gaussian_states(rng, n):
    st = np.zeros(n, abi.DSP_STATE)
    st.view(f32)[:] = rng.standard_normal(n * 8).astype(f32) * f32(0.1)
    return st


def make_inputs(kind, seed, params, frames, rows=None, raw=True, nf_sources=None, nf_samples=True):
    """Inputs of one value class for the sources `params` describes. Returns (samples float32 [rows, frames * 2],
    states abi.DSP_STATE [n], params, info): rows = n buffers (one per source) by default, or the T dry rows of a
    listener mix. `params` comes back as a crafted copy for the classes that set raw parameters (overflow, zeros,
    edge) when `raw`; with raw False the caller has built its sources so that they carry the class already.
    nf_sources / nf_samples: the sources that may get a non-finite state word, and whether samples get non-finite
    values at all (the dry rows of a mix are shared by every fan). info: what the class's condition needs."""
    assert kind in KINDS
    rng = np.random.default_rng(seed)
    n = params.size
    rows = n if rows is None else rows
    p = params.copy()
    info = {}
    stereo = np.flatnonzero((p["flags"] & 4) == 0)
    samples = (rng.standard_normal((rows, frames * 2)) * 0.5).astype(f32)
    states = _gaussian_states(rng, n)
    if kind == "tail":
        states.view(f32)[:] = log_uniform(rng, 1e-41, 1e-30, n * 8)
        samples = log_uniform(rng, 1e-44, 1e-36, (rows, frames * 2))
        samples[0::2] = 0
    elif kind == "nonfinite":
        vals = (f32(np.inf), f32(-np.inf), f32(np.nan))
        if nf_samples:
            for r in rng.choice(rows, max(3, rows // 10) if rows >= 3 else rows, replace=False):
                fr = int(rng.choice([f for f in {3, 64, frames - 1} if f < frames]))
                samples[r, 2 * fr + int(rng.integers(2))] = vals[int(rng.integers(3))]
        pool = stereo if nf_sources is None else np.intersect1d(stereo, nf_sources)
        hit = rng.choice(pool, min(3, pool.size), replace=False)
        for s in hit:  # in a word the source's class reads: previous_muffle, previous_lp, or previous_hp / previous_input
            fl = int(p["flags"][s])
            words = ([0, 1] if fl & 1 else []) + ([2, 3] if fl & 2 else [4, 5, 6, 7])
            states.view(f32).reshape(n, 8)[s, int(rng.choice(words))] = vals[int(rng.integers(3))]
        info["state_sources"] = np.sort(hit)
    elif kind == "overflow":
        samples = log_uniform(rng, 1e37, 3e38, (rows, frames * 2))
        if raw:
            p["volume"][stereo] = rng.uniform(2, 8, stereo.size).astype(f32)
            p["dry_boost"][stereo] = rng.uniform(2, 8, stereo.size).astype(f32)
    elif kind == "zeros":
        states = np.zeros(n, abi.DSP_STATE)
        samples = rng.choice(np.array([0.0, -0.0], f32), (rows, frames * 2))
        if raw:
            third = stereo[::3]
            neg = third[0::2]
            p["volume"][neg] = -np.abs(p["volume"][neg]) - f32(0.25)
            p["gain_left"][third[1::2]] = f32(-0.0)
    elif kind == "edge":
        assert raw, "edge parameters are raw parameters"
        k = stereo.size
        p["muffle_alpha"][stereo] = rng.choice(np.array(EDGE_ALPHAS, f32), k)
        p["filter_alpha"][stereo] = rng.choice(np.array(EDGE_ALPHAS, f32), k)
        p["dry_boost"][stereo] = rng.choice(np.array(EDGE_DRY_BOOSTS, f32), k)
        for name in ("gain_left", "gain_right"):
            g = rng.choice(np.array([0.0, -0.0, 1.0, np.nan], f32), k)  # nan: keep the source's own gain
            p[name][stereo] = np.where(np.isnan(g), p[name][stereo], g)
        if k:
            info["inf_volume"] = int(stereo[-1])
            p["volume"][stereo[-1]] = f32(np.inf)
        # the growing high pass: alpha 1.5 multiplies previous_hp by 1.5 per frame. 1.5^130 = 8e22, so from a
        # state of 1e18 the chain passes FLT_MAX (3.4e38) near frame 117
        hp = stereo[(p["flags"][stereo] & 2) == 0]
        hp = hp[hp != stereo[-1]] if k else hp
        if hp.size:
            s = int(hp[0])
            info["grower"] = s
            for name, v in (("filter_alpha", 1.5), ("muffle_alpha", 0.5), ("dry_boost", 1.0), ("gain_left", 1.0),
                            ("gain_right", 1.0), ("volume", 1.0)):
                p[name][s] = f32(v)
            states["previous_hp"][s] = (f32(1e18), f32(-1e18))
    return samples, states, p, info


def subnormal_share(a):
    v = np.abs(np.ascontiguousarray(a).view(f32).reshape(-1))
    return float(np.count_nonzero((v > 0) & (v < FLT_MIN_NORMAL))) / max(v.size, 1)


def check_condition(kind, params, samples, out, states_out, info):
    """The condition of a value class on the reference's own result (tests/test_dsp_chain_ref_cpu.py asserts these;
    without them a case could pass vacuously, for example on a host in flush-to-zero mode). `samples` has one row
    per source (the inputs the reference ran on)."""
    cls = np.where(params["flags"] & 4, 4, params["flags"] & 3)
    if kind == "tail":
        for c in sorted(set(cls.tolist()) - {4}):
            share = subnormal_share(out[cls == c])
            assert share >= 0.01, f"tail: class {c} has {share:.2%} subnormal output samples"
            assert subnormal_share(states_out[cls == c]) > 0, f"tail: class {c} leaves no subnormal state"
    elif kind == "overflow":
        assert np.isfinite(samples).all()
        assert np.isinf(out).any() and np.isnan(out).any(), "overflow: the chain gave no inf or no NaN from finite input"
    elif kind == "zeros":
        bits = set(np.unique(out[cls != 4].view(np.uint32)).tolist())
        assert {0x00000000, 0x80000000} <= bits, "zeros: the output does not hold both zeros"
    elif kind == "edge" and "grower" in info:
        s = info["grower"]
        assert params["filter_alpha"][s] == f32(1.5) and not params["flags"][s] & 2 and np.isfinite(params["volume"][s])
        assert np.isfinite(samples[s]).all() and np.isinf(out[s]).any(), "edge: alpha 1.5 on a high pass did not reach inf"
