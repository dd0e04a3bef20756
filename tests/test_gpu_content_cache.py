"""The content hash and the caches keyed by it: two clips never share visual tokens or prompt K/V.

Kernel part: o3v_content_hash128 against tests/hash_ref.py -- exact integers over the shared case list (every length at which the
launch takes another shape, one bit flipped anywhere from the first byte to the tail, the same words at other indices, zero bytes
that only the length tells apart), repeatability, address independence, the argument checks.

Cache part: vllm_api.LLM over the tiny / medium fixtures.  Every result is compared with a COLD run: a fresh LLM over a fresh engine,
nothing cached, the same request; greedy ids and counters exactly.  Clip B is golden clip A at the same shape and dtype, altered; the
alteration was picked on the CPU oracle (fp32, the golden prompt, the test's sampling parameters) as the candidate with the widest
top-1 / top-2 margin among {frames reversed, 255 - x, frames rolled by one, rows flipped, columns flipped, channels reversed} whose
greedy ids differ from A's:
    G7 medium  (frames as images)        B = 255 - x            oracle margin 0.166 (A: 0.090), ids differ from step 0
    G14 tiny   (native video)            B = frames rolled by 1  oracle margin 0.288 (A: 0.054), ids differ from step 1
    G12 tiny   (Qwen3-VL, frames)        B = columns flipped     oracle margin 0.363 (A: 0.244), ids differ from step 1
Each test first asserts cold(B) != cold(A): without it "B did not get A's answer" would hold vacuously."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fixture_models as fm
import fixture_models_q3 as fq
import hash_ref as hr
from test_gpu_facades import StubTokenizer
from test_gpu_model import build_engine
from test_gpu_video import VideoStubTokenizer, _prompt_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


# ----------------------------------------------------------------------------------------------------------------------------
# kernel
# ----------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _read(out):
    return tuple(int(v) & hr.M64 for v in out.tolist())


def device_hash(t: torch.Tensor, nbytes=None):
    """o3v_content_hash128 over the bytes of the device tensor `t` (its first `nbytes`), `out` zeroed before the call"""
    from open_o3_video_amd import _lib
    out = torch.zeros(2, dtype=torch.int64, device=t.device)
    _lib.call("o3v_content_hash128", C.c_void_p(t.data_ptr()), t.numel() * t.element_size() if nbytes is None else nbytes,
              C.c_void_p(out.data_ptr()), _stream())
    return _read(out)


def _to_dev(a: np.ndarray, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


@pytest.fixture(scope="module")
def hashed(dev):
    """name -> (reference value, device value) of every case, each computed once"""
    out = {}
    for c in hr.CASES:
        a = c.make()
        t = _to_dev(a, dev) if a.size else torch.zeros(8, dtype=torch.uint8, device=dev)     # an empty tensor has no address
        out[c.name] = (hr.content_hash128(a), device_hash(t, a.size))
    return out


def test_hash_equals_the_reference_exactly(hashed):
    bad = [(n, [hex(v) for v in got], [hex(v) for v in want]) for n, (want, got) in hashed.items() if got != want]
    assert not bad, f"{len(bad)} of {len(hashed)} cases differ (name, kernel, reference): {bad[:6]}"


def test_hash_tells_every_pair_apart(hashed):
    for p in hr.PAIRS:
        a, b = hashed[p.a][1], hashed[p.b][1]
        assert a[0] != b[0] and a[1] != b[1], f"{p.name}: {[hex(v) for v in a]} / {[hex(v) for v in b]}"


def test_hash_is_repeatable_and_address_independent(dev, hashed):
    a = hr.BY_NAME["random big"].make()
    want = hashed["random big"][0]
    t = _to_dev(a, dev)
    assert [device_hash(t) for _ in range(5)] == [want] * 5, "the atomics commute: one value whatever order the blocks arrive in"
    big = torch.zeros(a.size + 64, dtype=torch.uint8, device=dev)
    big[8:8 + a.size].copy_(t)
    view = big[8:8 + a.size]
    assert view.data_ptr() == big.data_ptr() + 8 and device_hash(view) == want
    # the small cases too, with other bytes right behind them (nothing past `bytes` may enter)
    for name in ("random 1", "random 9", "random 2047"):
        s = hr.BY_NAME[name].make()
        big.fill_(0xA5)
        big[8:8 + s.size].copy_(_to_dev(s, dev))
        assert device_hash(big[8:], s.size) == hashed[name][0], name


def test_hash_argument_checks(dev, hashed):
    from open_o3_video_amd import _lib
    t = _to_dev(hr.BY_NAME["random 2048"].make(), dev)
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    fn = _lib.load().o3v_content_hash128
    bad = {"null data": (C.c_void_p(None), 2048, C.c_void_p(out.data_ptr())),
           "null out": (C.c_void_p(t.data_ptr()), 2048, C.c_void_p(None)),
           "data 1 mod 8": (C.c_void_p(t.data_ptr() + 1), 2040, C.c_void_p(out.data_ptr()))}
    assert t.data_ptr() % 8 == 0
    for what, args in bad.items():
        assert fn(*args, _stream()) == _lib.ERR_ARG, what
        with pytest.raises(_lib.O3VError):
            _lib.call("o3v_content_hash128", *args, _stream())
        assert _read(out) == (0, 0), f"{what}: out written"
    # zero bytes behind a valid pointer: the empty buffer's value
    assert device_hash(t, 0) == hr.content_hash128(b"") == hashed["random 0"][0]


# ----------------------------------------------------------------------------------------------------------------------------
# caches
# ----------------------------------------------------------------------------------------------------------------------------
class Family:
    """One fixture model, its golden clip A and prompt, and how a request over a clip is written.  `warm`: the engine the tests
    share (each test starts from empty caches); cold(clip, **llm_kw): the ids of a fresh LLM over a fresh engine, memoised."""

    def __init__(self, name, cfg, W, tok, prompt, ids, A, B, kind, llm_kw, sp, engine_setup=None):
        self.name, self.cfg, self.W, self.tok, self.prompt, self.ids, self.A, self.B, self.kind = name, cfg, W, tok, prompt, ids, A, B, kind
        self.llm_kw, self.sp, self.engine_setup = llm_kw, sp, engine_setup
        self._cold = {}
        self.warm = self.engine()

    def engine(self):
        eng = build_engine(self.cfg, self.W)
        if self.engine_setup:
            self.engine_setup(eng)
        return eng

    def llm(self, eng=None, **kw):
        from open_o3_video_amd.vllm_api import LLM
        if eng is None:
            eng = self.warm
            eng.drop_prefix_cache()
            eng.drop_prompt_handover()
        return LLM(engine=eng, tokenizer=self.tok, max_model_len=4096, **{**self.llm_kw, **kw})

    def req(self, clip, kind=None):
        return {"prompt": self.prompt, "multi_modal_data": {kind or self.kind: clip}}

    def run(self, llm, clip):
        out = llm.generate(self.req(clip), self.sp)[0]
        assert out.prompt_token_ids == self.ids
        return out.outputs[0].token_ids

    def cold(self, clip, **kw):
        key = (hr.content_hash128(clip.numpy()), tuple(clip.shape), tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in self._cold:
            self._cold[key] = self.run(self.llm(self.engine(), **kw), clip)
        return self._cold[key]


def _image_prompt(cfg, ids):
    words, i = [], 0
    while i < len(ids):
        if ids[i] == cfg["image_token_id"]:
            words.append("<|image_pad|>")
            while i < len(ids) and ids[i] == cfg["image_token_id"]:
                i += 1
            continue
        words.append({cfg["vision_start_token_id"]: "<|vision_start|>", cfg["vision_end_token_id"]: "<|vision_end|>"}.get(ids[i], f"w{ids[i]}"))
        i += 1
    return " ".join(words)


@pytest.fixture(scope="module")
def image_fam(dev, golden_dir):
    from open_o3_video_amd.vllm_api import SamplingParams
    g = np.load(os.path.join(golden_dir, "g7_medium.npz"))
    cfg = fm.medium_config()
    ids = g["input_ids"][0].tolist()
    A = torch.from_numpy(g["frames"])
    sp = SamplingParams(temperature=0.0, repetition_penalty=1.05, max_tokens=16, stop_token_ids=[])
    f = Family("G7 medium", cfg, fm.make_weights(cfg, 2), StubTokenizer(cfg), _image_prompt(cfg, ids), ids, A, 255 - A, "image",
               dict(limit_mm_per_prompt={"image": 32}), sp)
    f.golden = g["bf16_ids_rp105"][0, len(ids):].tolist()
    return f


@pytest.fixture(scope="module")
def video_fam(dev, golden_dir):
    from open_o3_video_amd.vllm_api import SamplingParams
    g = np.load(os.path.join(golden_dir, "g14_video_tiny.npz"))
    cfg = fm.tiny_config()
    ids = g["input_ids"][0].tolist()
    A = torch.from_numpy(g["video_frames"])
    n_new = g["f32_step_logits"].shape[1]
    sp = SamplingParams(temperature=0.0, repetition_penalty=1.05, max_tokens=n_new, stop_token_ids=[])
    fps = 2.0 / float(g["second_per_grid_ts"][0])
    f = Family("G14 tiny", cfg, fm.make_weights(cfg, 0), VideoStubTokenizer(cfg), _prompt_text(cfg, ids, True), ids, A, torch.roll(A, 1, 0),
               "video", dict(limit_mm_per_prompt={"video": 10}, position_mode="tf5", mm_processor_kwargs={"fps": fps}), sp)
    f.golden = g["bf16_ids_rp105"][0, len(ids):].tolist()
    f.fps = fps
    return f


@pytest.fixture(scope="module")
def q3_fam(dev, golden_dir):
    from open_o3_video_amd.vllm_api import SamplingParams
    g = np.load(os.path.join(golden_dir, "g12_q3_tiny.npz"))
    cfg = fq.tiny_q3_config()
    ids = g["input_ids"][0].tolist()
    A = torch.from_numpy(g["frames"])
    sp = SamplingParams(temperature=0.0, max_tokens=g["f32_step_logits"].shape[1], stop_token_ids=[])
    f = Family("G12 Qwen3-VL tiny", cfg, fq.make_weights(cfg, 0), StubTokenizer(cfg), _image_prompt(cfg, ids), ids, A, torch.flip(A, dims=[3]),
               "image", dict(limit_mm_per_prompt={"image": 32}), sp)
    f.golden = g["bf16_ids"][0, len(ids):].tolist()
    return f


def _counters(llm):
    return llm.vis_cache_hits, llm.prefix_tokens_reused


@pytest.mark.parametrize("fam_name", ["image_fam", "video_fam", "q3_fam"])
def test_other_content_misses_then_the_first_clip_hits(request, fam_name):
    """A, then B under the same prompt (the same token ids: the prefix lookup alone would find a full match), then A again"""
    f = request.getfixturevalue(fam_name)
    cold_a, cold_b = f.cold(f.A), f.cold(f.B)
    assert cold_a == f.golden and cold_b != cold_a, "precondition: the two clips have different answers"
    llm = f.llm()
    assert f.run(llm, f.A) == cold_a and _counters(llm) == (0, 0)
    got_b = f.run(llm, f.B)
    assert _counters(llm) == (0, 0), "another clip of the same shape was served from the caches"
    assert got_b == cold_b
    got_a = f.run(llm, f.A)
    hits, reused = _counters(llm)
    assert hits == 1 and reused >= len(f.ids) - 1 and got_a == cold_a
    assert len(llm._vis_cache) == 2 and len(llm.engine._prefix) == 2


def test_one_bit_of_one_pixel_is_another_key(video_fam):
    """key level only: the ids of the two clips may well coincide"""
    f = video_fam
    A1 = f.A.clone()
    A1[-1, 2, -1, -1] ^= 1
    llm = f.llm()
    f.run(llm, f.A)
    f.run(llm, A1)
    assert _counters(llm) == (0, 0) and len(llm._vis_cache) == 2
    (ka, kb) = list(llm._vis_cache)
    assert ka[:-2] == kb[:-2] and ka[-2] != kb[-2] and ka[-1] != kb[-1], "same kind / shape / dtype / weights, both hash words differ"
    f.run(llm, A1)
    assert llm.vis_cache_hits == 1


@pytest.mark.parametrize("share", [False, True])
def test_one_call_over_two_clips(image_fam, share):
    """generate([A, B, A, B]), one prompt: every row its cold ids; with sharing on, two groups of two -- never one of four"""
    f = image_fam
    cold_a, cold_b = f.cold(f.A), f.cold(f.B)
    assert cold_b != cold_a
    llm = f.llm(share_video_prefix=share, max_num_seqs=8)
    outs = llm.generate([f.req(f.A), f.req(f.B), f.req(f.A), f.req(f.B)], f.sp)
    assert [o.outputs[0].token_ids for o in outs] == [cold_a, cold_b, cold_a, cold_b]
    assert llm.vis_cache_hits == 2 and len(llm._vis_cache) == 2          # rows 2 and 3 reuse the tokens of rows 0 and 1
    if share:
        assert (llm.shared_prefix_calls, llm.shared_prefix_rows) == (2, 4)
    else:
        assert (llm.shared_prefix_calls, llm.shared_prefix_rows) == (0, 0)


def test_shape_and_kind_are_part_of_the_key(video_fam):
    """the same bytes as [T,3,28,56] and as [T,3,56,28], and the same tensor as frames and as a video, miss each other"""
    f = video_fam
    g = torch.Generator().manual_seed(5)
    wide = torch.randint(0, 256, (2, 3, 28, 56), generator=g, dtype=torch.uint8)
    tall = wide.reshape(2, 3, 56, 28)
    assert torch.equal(wide.reshape(-1), tall.reshape(-1))
    from open_o3_video_amd.vllm_api import SamplingParams
    sp = SamplingParams(temperature=0.0, max_tokens=2, stop_token_ids=[])
    img = "w5 <|vision_start|><|image_pad|><|vision_end|> w6 <|vision_start|><|image_pad|><|vision_end|> w7 w8"
    vid = "w5 <|vision_start|><|video_pad|><|vision_end|> w7 w8"
    llm = f.llm(min_pixels=28 * 28, limit_mm_per_prompt={"image": 4, "video": 1})
    steps = [(img, {"image": wide}, 0), (img, {"image": tall}, 0), (vid, {"video": wide}, 0), (vid, {"video": tall}, 0),
             (img, {"image": tall}, 1), (vid, {"video": wide}, 2)]
    for k, (prompt, mm, hits) in enumerate(steps):
        out = llm.generate({"prompt": prompt, "multi_modal_data": mm}, sp)[0]
        assert len(out.outputs[0].token_ids) == 2
        assert llm.vis_cache_hits == hits, f"step {k}: {list(mm)} {tuple(next(iter(mm.values())).shape)}"
    keys = list(llm._vis_cache)
    assert len(keys) == 4 and len({k[-2:] for k in keys}) == 1, "four entries over one hash value: kind and shape told them apart"


def _rolled(f, k):
    return torch.roll(f.A, k, 0)


def test_visual_cache_holds_four_and_evicts_first_in_first_out(video_fam):
    f = video_fam
    llm = f.llm()
    assert llm.vis_cache_size == 4
    clips = [_rolled(f, k) for k in range(5)]
    assert len({hr.content_hash128(c.numpy()) for c in clips}) == 5
    first = []
    for c in clips:
        first.append(f.run(llm, c))
        assert len(llm._vis_cache) <= 4
    assert first[0] == f.cold(f.A) and llm.vis_cache_hits == 0
    assert f.run(llm, clips[0]) == first[0], "evicted: encoded again, the same ids"
    assert llm.vis_cache_hits == 0 and len(llm._vis_cache) == 4          # now [2, 3, 4, 0]: clip 1 left when clip 0 came back
    assert f.run(llm, clips[2]) == first[2] and llm.vis_cache_hits == 1
    assert f.run(llm, clips[1]) == first[1] and llm.vis_cache_hits == 1 and len(llm._vis_cache) == 4


def test_prefix_store_holds_two(video_fam):
    f = video_fam
    from open_o3_video_amd.engine import O3VEngine
    assert O3VEngine.PREFIX_ENTRIES == 2
    clips = [f.A, f.B, _rolled(f, 2)]
    cold = [f.cold(c) for c in clips]
    llm = f.llm()
    for c, want in zip(clips, cold):
        assert f.run(llm, c) == want
        assert len(llm.engine._prefix) <= 2
    assert _counters(llm) == (0, 0)
    assert f.run(llm, clips[0]) == cold[0]
    assert _counters(llm) == (1, 0), "the visual tokens were still cached, the prompt K/V were not"
    assert f.run(llm, clips[2]) == cold[2]
    assert llm.vis_cache_hits == 2 and llm.prefix_tokens_reused >= len(f.ids) - 1


def test_two_facades_over_one_engine_do_not_share_positions(video_fam):
    """The prompt K/V live on the engine and carry the M-RoPE positions they were rotated with: a facade with another position
    arithmetic, or other seconds per temporal patch, must not be served the K/V a first facade stored for the same clip and ids."""
    f = video_fam
    eng = f.warm
    one = f.llm()                                                                               # tf5, the golden's fps
    settings = [dict(position_mode="pinned", mm_processor_kwargs={"fps": 2.0}),                # the facade's defaults
                dict(position_mode="tf5", mm_processor_kwargs={"fps": f.fps / 2})]             # the seconds alone
    colds = [f.cold(f.A, **kw) for kw in settings]
    cold_one = f.cold(f.A)
    assert cold_one == f.golden
    assert all(c != cold_one for c in colds), "precondition: the settings change the answer"
    assert f.run(one, f.A) == cold_one
    for kw, want in zip(settings, colds):
        other = f.llm(eng, **kw)
        assert f.run(other, f.A) == want, kw
        assert f.run(other, f.A) == want and other.prefix_tokens_reused >= len(f.ids) - 1, "its own second run does reuse"
    assert f.run(one, f.A) == cold_one


def test_device_frames_at_an_unaligned_address(video_fam):
    """frames that already live on the device, contiguous, 4 bytes into an allocation: hashed (from an aligned copy), not refused"""
    f = video_fam
    n = f.A.numel()
    buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
    view = buf[4:4 + n].view(f.A.shape)
    view.copy_(f.A)
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    assert view.to("cuda").contiguous().data_ptr() == view.data_ptr(), "precondition: nothing on the way copies the view"
    llm = f.llm()
    aligned = f.run(llm, f.A)
    assert aligned == f.cold(f.A)
    assert f.run(llm, view) == aligned and llm.vis_cache_hits == 1, "the same bytes: the same key"
    llm2 = f.llm()
    assert f.run(llm2, view) == aligned and f.run(llm2, view) == aligned and llm2.vis_cache_hits == 1
