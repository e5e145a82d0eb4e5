"""The NumPy float32 reference of the per-sample chain (tests/dsp_chain_ref.py) against the oracle's restatement of
AudioSpatializer.OnAudioFilterRead and against the listener mix's host twin (art_dsp_mix_host), bit for bit, on
every value class; the conditions that keep the value classes from passing vacuously; and one hand-derived answer.
No GPU: tests/test_dsp_variants_gpu.py holds the kernels to the same reference.
"""
import numpy as np
import pytest

import art
from art import abi
from art.dsp import SpatializerSettings
import dsp_chain_ref as ref
import oracle

f32 = np.float32
PER_CLASS = 32
CLASSES = [c for c in range(4) for _ in range(PER_CLASS)]


def oracle_case(kind, frames, seed):
    """128 sources, 32 per filter class, built so that art.dsp.source_params carries the value class: the overflow
    class's volume and dry boost in [2, 8], a third of the zeros class's volumes negative."""
    rng = np.random.default_rng(seed)
    st = SpatializerSettings()
    srcs = ref.class_sources(rng, CLASSES, frames, volume=(2.0, 8.0) if kind == "overflow" else (0.0, 2.0))
    if kind == "overflow":
        st.reverb_dry_boost = (2.0, 8.0)
    if kind == "zeros":
        for s in srcs[::3]:
            s.volume_multiplier = -s.volume_multiplier - 0.25
    params = np.concatenate([art.dsp.source_params(st, s, 48000) for s in srcs])
    assert ((params["flags"] & 7) == np.asarray(CLASSES)).all()
    return st, srcs, params


@pytest.mark.parametrize("frames", [1, 64, 65, 130])
@pytest.mark.parametrize("kind", ["gaussian", "tail", "nonfinite", "overflow", "zeros"])
def test_reference_equals_oracle(kind, frames):
    """Two calls with the state carried, all four filter classes, parameters from art.dsp.source_params. The tail,
    overflow and zeros conditions are asserted on the reference's result (the first two at 65 and 130 frames)."""
    st, srcs, params = oracle_case(kind, frames, 1000 + frames)
    states = None
    for call in range(2):
        samples, fresh, _, info = ref.make_inputs(kind, 10 * frames + call, params, frames, raw=False)
        if call == 0:
            states = fresh
            for s, src in enumerate(srcs):
                src.state = states[s:s + 1].copy()
        for s, src in enumerate(srcs):
            src.data = samples[s].copy()
        want, want_states = ref.chain(params, states, samples)
        oracle.dsp_process(st, srcs, 48000)
        ref.assert_same_bits(np.stack([s.data for s in srcs]), want, f"{kind} call {call} data")
        ref.assert_same_bits(np.concatenate([s.state for s in srcs]), want_states, f"{kind} call {call} state")
        # (a NaN needs an inf in the state first, and the tail's shares were measured at 65 and 130 frames)
        if call == 0 and (kind == "zeros" or frames >= 65):
            ref.check_condition(kind, params, samples, want, want_states, info)
        if kind == "overflow":
            assert (params["dry_boost"] >= 2).all() and (params["volume"] >= 2).all()
        states = want_states


def raw_case(kind, n_classes, frames, seed, rows=None, **kw):
    rng = np.random.default_rng(seed)
    params = ref.class_params(rng, n_classes)
    return ref.make_inputs(kind, seed + 1, params, frames, rows=rows, **kw)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_reference_equals_mix_host_single_target(kind):
    """T = 1: the mix is the chain itself. 130 frames, 32 sources per class, raw parameters (edge included); every
    condition of the value classes is asserted here on the reference alone."""
    frames, F = 130, len(CLASSES)
    samples, states, params, info = raw_case(kind, CLASSES, frames, 77)
    want, want_states = ref.chain(params, states, samples)
    ref.check_condition(kind, params, samples, want, want_states, info)
    if kind == "nonfinite":
        assert not np.isfinite(samples).all() and not np.isfinite(states.view(f32)).all()
    if kind == "edge":
        for name in ("muffle_alpha", "filter_alpha"):
            assert set(np.unique(params[name].view(np.uint32))) == set(np.array(ref.EDGE_ALPHAS, f32).view(np.uint32).tolist())
        assert {0x00000000, 0x80000000} <= set(params["gain_left"].view(np.uint32).tolist())
        assert np.isinf(params["volume"]).sum() == 1
    # a fan of one target: fan f hears source f over dry row 0, so run the sources one fan at a time
    got = np.empty_like(want)
    got_states = states.copy()
    for s in range(F):
        got[s] = art.dsp.mix_host(params[s:s + 1], got_states[s:s + 1], samples[s:s + 1], 1, 1)[0]
    ref.assert_same_bits(got, want, f"{kind} mix at T = 1")
    ref.assert_same_bits(got_states, want_states, f"{kind} state at T = 1")


@pytest.mark.parametrize("F,T,frames", [(3, 5, 65), (2, 33, 130)])
@pytest.mark.parametrize("kind", ref.KINDS)
def test_reference_mix_equals_mix_host(kind, F, T, frames):
    """The ordered sum on top of the chain, two calls with the state carried, mixed classes in a fan."""
    rng = np.random.default_rng(100 * F + T)
    classes = rng.integers(0, 4, F * T).tolist()
    classes[T // 2] = 4  # one source that is not stereo: its dry frames as they are
    params0 = ref.class_params(rng, classes)
    states = None
    for call in range(2):
        dry, fresh, params, _ = ref.make_inputs(kind, 31 * T + call, params0, frames, rows=T,
                                                nf_sources=np.arange(T, 2 * T), nf_samples=False)
        states = fresh if call == 0 else states
        want, want_states = ref.mix(params, states, dry, F, T)
        got_states = states.copy()
        got = art.dsp.mix_host(params, got_states, dry, F, T)
        ref.assert_same_bits(got, want, f"{kind} call {call} mix")
        ref.assert_same_bits(got_states, want_states, f"{kind} call {call} state")
        states = want_states


def test_assert_same_bits_rules():
    a = np.array([[0.0, -0.0, np.nan, 1.0]], f32)
    b = a.copy()
    b.view(np.uint32)[0, 2] ^= 0x80000001  # another NaN: sign and payload are free
    ref.assert_same_bits(b, a, "nan payload")
    for k, v in ((0, f32(-0.0)), (2, f32(1.0)), (3, f32(np.nan)), (3, np.nextafter(f32(1), f32(2)))):
        c = a.copy()
        c[0, k] = v
        with pytest.raises(AssertionError, match=f"source 0, frame {k // 2}, channel {k % 2}"):
            ref.assert_same_bits(c, a, "changed")
    s = np.zeros(3, abi.DSP_STATE)
    t = s.copy()
    t["previous_hp"][2, 1] = 1e-45
    with pytest.raises(AssertionError, match="source 2, state word previous_hp channel 1"):
        ref.assert_same_bits(t, s, "state")


def test_known_answer_low_pass_decays_through_the_subnormals():
    """Derived by hand, from no implementation. A class 2 source (no muffle, low pass) with alpha = 0.5, dry boost,
    gains and volume 1, zero input and previous_lp = 2^-125. The input reaches the filter as 0 * 1 * 1 = 0, and
    pl' = pl + 0.5 * (0 - pl), each operation rounded to float32:
      step 1: 0 - 2^-125 = -2^-125; 0.5 * -2^-125 = -2^-126; 2^-125 + -2^-126 = 2^-126, the smallest normal number;
      step 2: 0 - 2^-126 = -2^-126; 0.5 * -2^-126 = -2^-127, a subnormal, exact (one mantissa bit);
              2^-126 + -2^-127 = 2^-127.
    Every further step halves exactly, down to 2^-149, the smallest subnormal (step 24). Then 0.5 * -2^-149 = -2^-150
    lies halfway between -0 and -2^-149 and rounds to even, that is to -0, and 2^-149 + -0 = 2^-149: the value stays
    forever. The output of step k is pl times the volume 1: bits 0x00800000 >> (k - 1), and 1 from step 24 on. A chain
    that flushes subnormals gives 0 from step 2 on."""
    frames = 40
    want_bits = np.array([max(0x00800000 >> k, 1) for k in range(frames)], np.uint32)
    assert want_bits[0] == 0x00800000 and want_bits[1] == 0x00400000 and want_bits[23] == 1 and want_bits[39] == 1
    p = np.zeros(1, abi.DSP_SOURCE_PARAMS)
    p["flags"], p["filter_alpha"] = 2, 0.5
    p["muffle_alpha"] = 0.5
    for name in ("dry_boost", "gain_left", "gain_right", "volume"):
        p[name] = 1.0
    st = np.zeros(1, abi.DSP_STATE)
    st["previous_lp"] = np.array([0x01000000, 0x01000000], np.uint32).view(f32)  # 2^-125
    assert st["previous_lp"][0, 0] == f32(2.0) ** -125
    x = np.zeros((1, frames * 2), f32)
    out, new = ref.chain(p, st, x)
    assert (out.view(np.uint32).reshape(frames, 2) == want_bits[:, None]).all()
    assert new["previous_lp"].view(np.uint32).tolist() == [[1, 1]] and new["previous_muffle"].tolist() == [[0, 0]]
    host_state = st.copy()
    got = art.dsp.mix_host(p, host_state, x, 1, 1)
    assert (got.view(np.uint32).reshape(frames, 2) == want_bits[:, None]).all()
    assert host_state.tobytes() == new.tobytes()
