"""The T5 per-token generation step on the GPU: the two decode-attention
kernels (csrc/s2s_decode.hip) against their fp32 references on the same bf16
inputs, their host checks, ``decode_step`` against the full-sequence forward,
and the graph engine against the same kernels in a plain loop (token equality,
bit for bit: both run the same arithmetic).

The tolerance is the project's 3e-2 for bf16-in / fp32-accumulate attention
kernels against the fp32 reference (test_t5_attention_gpu.py).  Bias tables
are N(0, 1) per head, so a bias index off by one moves the output by more than
that (asserted on the reference alone)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from trlx_amd import ops
    from trlx_amd.ops import reference

DEV = "cuda"
TOL = dict(atol=3e-2, rtol=3e-2)
B, H, S = 3, 4, 80
# one key only; either side of the keys-per-block-iteration stride (16 at
# D=128, 32 at D=64); the last slot
POSITIONS = (0, 1, 15, 16, 17, 31, 32, 33, 79)


def _rand(*shape):
    return (torch.randn(*shape, device=DEV) * 0.5).bfloat16()


# ---- self-attention step ----------------------------------------------------------


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bias", [False, True])
def test_self_step_matches_reference_and_appends_in_place(D, bias):
    torch.manual_seed(D + bias)
    kc, vc = _rand(B, H, S, D), _rand(B, H, S, D)
    vec, zero = None, 0
    if bias:
        table = torch.randn(32, H, device=DEV)  # N(0, 1)
        vec, zero = ops.t5_rel_bias(table, 1, 1, S - 1, False)
        assert vec.shape == (H, S) and zero == S - 1
    cache_idx = torch.zeros(1, dtype=torch.long, device=DEV)
    at = 0
    for pos in POSITIONS:
        cache_idx += pos - at  # in place, on the device: same tensors, next position
        at = pos
        q, kn, vn = _rand(B, H, D), _rand(B, H, D), _rand(B, H, D)
        kc0, vc0 = kc.clone(), vc.clone()
        out = ops.seq2seq_decode_attention(q, kn, vn, kc, vc, cache_idx, rel_bias=vec,
                                           bias_zero=zero, scale=0.25)
        assert out.shape == (B, H, 1, D) and out.dtype == torch.bfloat16
        # row pos is the new token, bit for bit; every other row is untouched
        assert torch.equal(kc[:, :, pos], kn) and torch.equal(vc[:, :, pos], vn), pos
        keep = torch.arange(S, device=DEV) != pos
        assert torch.equal(kc[:, :, keep], kc0[:, :, keep]), pos
        assert torch.equal(vc[:, :, keep], vc0[:, :, keep]), pos
        rk, rv = kc0.clone(), vc0.clone()
        want = reference.seq2seq_decode_attention(q, kn, vn, rk, rv, cache_idx, vec, zero, 0.25)
        assert torch.equal(rk, kc) and torch.equal(rv, vc)  # same append semantics
        torch.testing.assert_close(out.float(), want.float(), **TOL, msg=lambda m: f"pos {pos}: {m}")
        if bias and pos == 33:  # an index error of one would show
            off = reference.seq2seq_decode_attention(q, kn, vn, rk, rv, cache_idx, vec, zero - 1,
                                                     0.25)
            assert (off.float() - want.float()).abs().max() > 3e-2
    assert int(cache_idx) == POSITIONS[-1]


@pytest.mark.parametrize("bad", [-1, S, 2**40])
def test_self_step_out_of_range_index_touches_nothing(bad):
    D = 64
    q, kn, vn = _rand(B, H, D), _rand(B, H, D), _rand(B, H, D)
    kc, vc = _rand(B, H, S, D), _rand(B, H, S, D)
    kc0, vc0 = kc.clone(), vc.clone()
    idx = torch.full((1,), bad, dtype=torch.long, device=DEV)
    out = ops.seq2seq_decode_attention(q, kn, vn, kc, vc, idx)
    assert torch.equal(out, torch.zeros_like(out))
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)


# ---- cross-attention step ---------------------------------------------------------


def _mask(kind, Tk):
    if kind == "none":
        return None
    m = torch.ones(B, Tk, dtype=torch.uint8, device=DEV)
    if kind == "right":
        m[0, Tk - Tk // 4:] = 0
        m[1, Tk // 2:] = 0
    elif kind == "left":
        m[0, : Tk // 2] = 0
        m[2, : Tk - 1] = 0  # one visible key, the last
    elif kind == "holes":
        g = torch.Generator().manual_seed(7)
        m = (torch.rand(B, Tk, generator=g) > 0.4).to(torch.uint8).to(DEV)
        m[:, Tk // 2] = 1
    elif kind == "dead":  # one all-masked row
        m[1] = 0
        m[2, ::2] = 0
    return m


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Tk", [1, 37, 130])
@pytest.mark.parametrize("kind", ["none", "right", "left", "holes", "dead"])
def test_cross_step_matches_reference(D, Tk, kind):
    torch.manual_seed(Tk)
    q, k, v = _rand(B, H, 1, D), _rand(B, H, Tk, D), _rand(B, H, Tk, D)
    mask = _mask(kind, Tk)
    if mask is not None:  # what lies behind the mask must not leak: NaN rows
        hidden = (mask == 0)[:, None, :, None].expand_as(k)
        k = torch.where(hidden, torch.full_like(k, float("nan")), k)
        v = torch.where(hidden, torch.full_like(v, float("nan")), v)
    out = ops.seq2seq_cross_decode_attention(q, k, v, key_mask=mask, scale=0.25)
    assert out.shape == (B, H, 1, D) and out.dtype == torch.bfloat16
    assert torch.isfinite(out).all()
    want = reference.seq2seq_cross_decode_attention(q, k, v, mask, 0.25)
    assert torch.isfinite(want).all()
    torch.testing.assert_close(out.float(), want.float(), **TOL)
    if mask is not None:
        for b in range(B):
            if not mask[b].any():  # no visible key: zeros
                assert torch.equal(out[b], torch.zeros_like(out[b]))
    if kind == "holes" and Tk > 1:  # the mask matters: ignoring it moves the output
        clean_k, clean_v = torch.nan_to_num(k, nan=2.0), torch.nan_to_num(v, nan=2.0)
        leaked = reference.seq2seq_cross_decode_attention(q, clean_k, clean_v, None, 0.25)
        assert (leaked.float() - want.float()).abs().max() > 3e-2


# ---- host checks ------------------------------------------------------------------


def _self_args(D=64, b=B):
    return dict(q=_rand(b, H, D), k_new=_rand(b, H, D), v_new=_rand(b, H, D),
                k_cache=_rand(b, H, S, D), v_cache=_rand(b, H, S, D),
                cache_idx=torch.zeros(1, dtype=torch.long, device=DEV))


def _ext():
    return ops._load_ext()


@pytest.mark.parametrize("change, message", [
    (lambda a: a.update(q=a["q"].float()), "q must be bf16"),
    (lambda a: a.update(k_cache=a["k_cache"].half()), "k_cache must be bf16"),
    (lambda a: a.update(v_new=a["v_new"].cpu()), "v_new must live on the same GPU"),
    (lambda a: a.update(k_cache=a["k_cache"].transpose(0, 1).contiguous().transpose(0, 1)),
     "k_cache must be contiguous"),
    (lambda a: a.update(k_new=_rand(B, H, 32)), "k_new and v_new must have q's shape"),
    (lambda a: a.update(v_cache=_rand(B, H, S + 1, 64)), "v_cache must have k_cache's shape"),
    (lambda a: a.update(k_cache=_rand(B, 2, S, 64), v_cache=_rand(B, 2, S, 64)),
     "no grouped heads"),
    (lambda a: a.update(cache_idx=torch.zeros(1, dtype=torch.long)), "cache_idx must be"),
    (lambda a: a.update(cache_idx=torch.zeros(1, dtype=torch.int32, device=DEV)),
     "cache_idx must be"),
    (lambda a: a.update(cache_idx=torch.zeros(2, dtype=torch.long, device=DEV)),
     "cache_idx must be"),
    (lambda a: a.update(rel_bias=torch.zeros(H, S, device=DEV).bfloat16()),
     r"rel_bias must be contiguous fp32 \[H, L\]"),
    (lambda a: a.update(rel_bias=torch.zeros(H + 1, S, device=DEV)),
     r"rel_bias must be contiguous fp32 \[H, L\]"),
    (lambda a: a.update(rel_bias=torch.zeros(H, S)), "rel_bias must live on the same device"),
    (lambda a: a.update(rel_bias=torch.zeros(H, S, device=DEV), bias_zero=S), "bias_zero"),
])
def test_self_step_host_checks(change, message):
    args = _self_args()
    change(args)
    with pytest.raises(RuntimeError, match=message):
        _ext().seq2seq_decode_attention(**args)


@pytest.mark.parametrize("change, message", [
    (lambda a: a.update(q=a["q"].float()), "q must be bf16"),
    (lambda a: a.update(v=a["v"].cpu()), "v must live on the same GPU"),
    (lambda a: a.update(k=a["k"].transpose(1, 2).contiguous().transpose(1, 2)),
     "k must be contiguous"),
    (lambda a: a.update(q=_rand(B, H, 2, 64)), r"q must be \[B, H, 1, D\]"),
    (lambda a: a.update(k=_rand(B, 2, 37, 64), v=_rand(B, 2, 37, 64)), "no grouped heads"),
    (lambda a: a.update(key_mask=torch.ones(B, 37, dtype=torch.bool, device=DEV)),
     r"key_mask must be contiguous uint8 \[B, Tk\]"),
    (lambda a: a.update(key_mask=torch.ones(B, 36, dtype=torch.uint8, device=DEV)),
     r"key_mask must be contiguous uint8 \[B, Tk\]"),
    (lambda a: a.update(key_mask=torch.ones(B, 37, dtype=torch.uint8)),
     "key_mask must live on the same device"),
])
def test_cross_step_host_checks(change, message):
    args = dict(q=_rand(B, H, 1, 64), k=_rand(B, H, 37, 64), v=_rand(B, H, 37, 64))
    change(args)
    with pytest.raises(RuntimeError, match=message):
        _ext().seq2seq_cross_decode_attention(**args)


@pytest.mark.parametrize("D", [32, 96, 256])
def test_unsupported_head_dim_names_the_supported_ones(D):
    with pytest.raises(RuntimeError, match=f"head dim must be 64 or 128, got {D}"):
        _ext().seq2seq_decode_attention(**_self_args(D))
    with pytest.raises(RuntimeError, match=f"head dim must be 64 or 128, got {D}"):
        _ext().seq2seq_cross_decode_attention(_rand(B, H, 1, D), _rand(B, H, 5, D),
                                              _rand(B, H, 5, D))


def test_empty_batch_returns_empty():
    out = _ext().seq2seq_decode_attention(**_self_args(b=0))
    assert out.shape == (0, H, 1, 64)
    out = _ext().seq2seq_cross_decode_attention(_rand(0, H, 1, 64), _rand(0, H, 5, 64),
                                                _rand(0, H, 5, 64))
    assert out.shape == (0, H, 1, 64)


# ---- model level ------------------------------------------------------------------


def _tiny_t5(tied=True):
    """The recipe of test_t5_attention_gpu.py::_tiny_t5: unit embeddings,
    sharpened q/k and N(0, 1) bias tables make the comparisons bite.

    Through the tied head that model's own token wins every argmax by ten
    logits (|e|^2 / sqrt(d_model) against N(0, 1)), so greedy decoding repeats
    the start token.  ``tied=False`` is the same recipe with an untied N(0, 1)
    head and the v / o projections of every decoder attention times 8, so that
    the attention outputs outweigh the token's own embedding: its greedy tokens
    vary from step to step and from prompt to prompt (asserted), and an engine
    that decoded a stale or wrong state could not hide behind a sequence that
    ignores the caches, the mask or the prompt."""
    from trlx_amd.models.nn.seq2seq import Seq2SeqConfig, Seq2SeqTransformer

    # seed 24: a draw whose greedy sequences are not fixed points of the argmax
    # (seed 4, untied, answers every token with token 0)
    torch.manual_seed(4 if tied else 24)
    cfg = Seq2SeqConfig(vocab_size=96, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2,
                        tie_word_embeddings=tied)
    model = Seq2SeqTransformer(cfg)
    model.shared.weight.data.normal_(0.0, 1.0)
    if not tied:
        model.lm_head.weight.data.normal_(0.0, 1.0)
        for blk in model.decoder_blocks:
            for attn in (blk.self_attn, blk.cross_attn):
                attn.v.weight.data.mul_(8.0)
                attn.o.weight.data.mul_(8.0)
    for blocks in (model.encoder_blocks, model.decoder_blocks):
        blocks[0].self_attn.relative_attention_bias.weight.data.normal_(0.0, 1.0)
        for blk in blocks:
            blk.self_attn.q.weight.data.mul_(4.0)
            blk.self_attn.k.weight.data.mul_(4.0)
    return model.to(DEV).bfloat16().eval(), cfg


def _prompts(cfg, T=37):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(2, cfg.vocab_size, (3, T), generator=g).to(DEV)
    mask = torch.ones_like(ids)
    mask[0, :9] = 0           # left pad
    mask[1, T - 7:] = 0       # right pad
    return ids, mask


def _plain(monkeypatch, model, *args, **kwargs):
    """The same kernels in a plain Python loop, no graph."""
    monkeypatch.setenv("TRLX_AMD_NO_GRAPHS", "1")
    try:
        return model.generate(*args, **kwargs)
    finally:
        monkeypatch.delenv("TRLX_AMD_NO_GRAPHS")


def test_decode_step_matches_full_forward_teacher_forced():
    model, cfg = _tiny_t5()
    ids, mask = _prompts(cfg)
    g = torch.Generator().manual_seed(6)
    dec = torch.randint(2, cfg.vocab_size, (3, 21), generator=g).to(DEV)
    with torch.no_grad():
        full = model(ids, mask, dec).logits.float()
        enc = model.encode(ids, mask)
        state = model.new_decode_state(3, enc_capacity=40, max_positions=24)
        state.begin(model, enc, mask)
        steps = []
        for t in range(dec.shape[1]):
            steps.append(model.project(model.decode_step(dec[:, t:t + 1], state)))
            state.cache_idx += 1
    stepped = torch.cat(steps, dim=1).float()
    assert full.abs().max() > 10 * 3e-2  # the comparison is not about zeros
    torch.testing.assert_close(stepped, full, **TOL)


def _varied(tokens):
    """Do the generated tokens (column 0 is the start token) vary along each
    row, and between the rows (whose prompts differ)?"""
    rows = [tuple(row[1:].tolist()) for row in tokens]
    return all(len(set(row)) >= 4 for row in rows) and len(set(rows)) == len(rows)


@pytest.mark.parametrize("tied", [True, False])
def test_graph_engine_matches_plain_loop_greedy(monkeypatch, tied):
    from trlx_amd.models.nn.generation import Seq2SeqDecodeEngine

    model, cfg = _tiny_t5(tied)
    ids, mask = _prompts(cfg)
    kw = dict(max_new_tokens=9, do_sample=False, eos_token_id=cfg.vocab_size + 5)
    assert getattr(model, "_decode_engine", None) is None
    out = model.generate(ids, mask, **kw)
    engine = model._decode_engine
    assert isinstance(engine, Seq2SeqDecodeEngine) and engine.graph is not None
    assert out.shape == (3, 10) and (out[:, 0] == cfg.decoder_start_token_id).all()
    assert tied or _varied(out)
    plain = _plain(monkeypatch, model, ids, mask, **kw)
    assert torch.equal(out, plain)
    # a second call: the same engine, the same graph, the same tokens
    graph = engine.graph
    assert torch.equal(model.generate(ids, mask, **kw), out)
    assert model._decode_engine is engine and engine.graph is graph
    # a shorter prompt reuses them too
    ids20, mask20 = _prompts(cfg, T=20)
    short = model.generate(ids20, mask20, **kw)
    assert model._decode_engine is engine and engine.graph is graph
    assert torch.equal(short, _plain(monkeypatch, model, ids20, mask20, **kw))
    assert tied or not torch.equal(short, out)
    assert model._decode_engine is engine
    # and the long prompt again, after the short one wrote the buffers
    assert torch.equal(model.generate(ids, mask, **kw), out)


def test_graph_engine_matches_plain_loop_sampling(monkeypatch):
    model, cfg = _tiny_t5()
    ids, mask = _prompts(cfg)
    # temperature 4 flattens the tied head's ten-logit margin: the samples vary
    kw = dict(max_new_tokens=9, do_sample=True, seed=7, temperature=4.0,
              eos_token_id=cfg.vocab_size + 5)
    out = model.generate(ids, mask, **kw)
    assert model._decode_engine.graph is not None and _varied(out)
    assert torch.equal(out, _plain(monkeypatch, model, ids, mask, **kw))
    assert torch.equal(out, model.generate(ids, mask, **kw))  # explicit seed: repeatable
    other = model.generate(ids, mask, **dict(kw, seed=8))
    assert not torch.equal(other, out)
    assert torch.equal(other, _plain(monkeypatch, model, ids, mask, **dict(kw, seed=8)))


@pytest.mark.parametrize("tied", [True, False])
def test_eos_pads_the_row_and_trims_like_the_plain_loop(monkeypatch, tied):
    model, cfg = _tiny_t5(tied)
    ids, mask = _prompts(cfg)
    free = model.generate(ids, mask, max_new_tokens=9, do_sample=False,
                          eos_token_id=cfg.vocab_size + 5)
    eos = int(free[0, 3])  # what row 0 emitted at step 3
    first = int((free[0, 1:] == eos).nonzero()[0]) + 1  # it may have come earlier too
    pad = 1  # a token of the vocabulary (a finished row feeds it back in) the prompts never use
    kw = dict(max_new_tokens=9, do_sample=False, eos_token_id=eos, pad_token_id=pad)
    out = model.generate(ids, mask, **kw)
    assert model._decode_engine.graph is not None
    assert torch.equal(out[0, : first + 1], free[0, : first + 1])
    assert (out[0, first + 1:] == pad).all()  # padded from there on
    # the width, predicted from the run without EOS: the last row to emit it decides
    ends = [(row[1:] == eos).nonzero() for row in free]
    assert out.shape[1] == 1 + max(int(e[0]) + 1 if len(e) else 9 for e in ends)
    for r, e in enumerate(ends):  # each row: its free-running tokens up to its EOS
        n = int(e[0]) + 2 if len(e) else out.shape[1]
        assert torch.equal(out[r, :n], free[r, :n]) and (out[r, n:] == pad).all()
    plain = _plain(monkeypatch, model, ids, mask, **kw)
    assert out.shape == plain.shape and torch.equal(out, plain)
    # one row only (a batch of its own: the GEMMs may round differently, so only
    # its own plain loop is the yardstick): the width is where that row finished
    one = model.generate(ids[:1], mask[:1], **kw)
    assert torch.equal(one, _plain(monkeypatch, model, ids[:1], mask[:1], **kw))
    hits = (one[0, 1:] == eos).nonzero()
    assert one.shape[1] == (int(hits[0]) + 2 if len(hits) else 10)


@pytest.mark.parametrize("tied", [True, False])
def test_in_place_training_between_calls_reaches_the_graph(monkeypatch, tied):
    """The stale-bias-vector test.  Tokens: the engine's next call equals a
    fresh model's plain loop, and differs from its previous output — the latter
    on the untied model only: the tied recipe's greedy output is the start
    token repeated whatever the attention does (a ten-logit margin, see
    ``_tiny_t5``), so no noise on the bias table and one q projection can move
    it.  On both models the bias vector the graph reads is checked directly:
    same buffer, new contents, equal to the vector of the trained table."""
    model, cfg = _tiny_t5(tied)
    ids, mask = _prompts(cfg)
    kw = dict(max_new_tokens=9, do_sample=False, eos_token_id=cfg.vocab_size + 5)
    before = model.generate(ids, mask, **kw)
    engine = model._decode_engine
    graph = engine.graph
    vec_before, vec_ptr = engine.state.rel_bias.clone(), engine.state.rel_bias.data_ptr()
    with torch.no_grad():
        torch.manual_seed(11)
        table = model.decoder_blocks[0].self_attn.relative_attention_bias.weight
        table.add_(torch.randn_like(table) * 2.0)
        qw = model.decoder_blocks[1].self_attn.q.weight
        qw.add_(torch.randn_like(qw) * 0.1)
    after = model.generate(ids, mask, **kw)
    assert model._decode_engine is engine and engine.graph is graph  # no re-capture
    # a fresh model with the trained weights, no engine, plain loop
    fresh, _ = _tiny_t5(tied)
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(after, _plain(monkeypatch, fresh, ids, mask, **kw))
    assert tied or not torch.equal(after, before)
    want, zero = ops.t5_rel_bias(table, 1, 1, engine.state.max_positions - 1, False)
    assert engine.state.rel_bias.data_ptr() == vec_ptr and zero == engine.state.bias_zero
    assert torch.equal(engine.state.rel_bias, want)
    assert (engine.state.rel_bias - vec_before).abs().max() > 1.0
    # the bias table alone reaches the graph as well (the stale-vector case)
    with torch.no_grad():
        table.add_(torch.randn_like(table) * 2.0)
    fresh.load_state_dict(model.state_dict())
    again = model.generate(ids, mask, **kw)
    assert torch.equal(again, _plain(monkeypatch, fresh, ids, mask, **kw))
    assert tied or not torch.equal(again, after)
    assert torch.equal(engine.state.rel_bias,
                       ops.t5_rel_bias(table, 1, 1, engine.state.max_positions - 1, False)[0])


def test_escape_hatch_keeps_the_old_loop(monkeypatch):
    model, cfg = _tiny_t5()
    ids, mask = _prompts(cfg)
    monkeypatch.setenv("TRLX_AMD_NO_S2S_DECODE", "1")
    out = model.generate(ids, mask, max_new_tokens=5, do_sample=False,
                         eos_token_id=cfg.vocab_size + 5)
    assert out.shape == (3, 6)
    assert getattr(model, "_decode_engine", None) is None
