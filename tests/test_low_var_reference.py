"""The systematic resampler's stream against the reference and against torch itself, on the CPU.

G19 (tools/gen_loop_trace_low_var.py) is G13's loop with `pf.resampler(parts, resample="low_var")` (particle_filter.py:251-261,
288-307): per frame torch.manual_seed(3000 + t), torch.normal tn, rot, then ONE float32 `torch.rand(1)` - the offset.  Here:
the oracle's systematic search fed the stored offsets replays the reference's indices in every frame; torch reproduces the stored
offsets under the stored seeds; the generator's position around the draw is what the draw sizes say; and the value and word
accounting of the device generator's `rand32` draw kind (csrc/mt19937.hip mt_u24: one output, low 24 bits x 2^-24) are pinned
against torch's generator state itself, with the host bookkeeping of torch_rng.py (rand32_words, skip_rand32, the state hand-over)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from _recipes import sha  # noqa: E402


def _check_digest(g, key, a):
    a = np.ascontiguousarray(a)
    assert np.array_equal(a[:32], g[key + "_head"]) and np.array_equal(a[-32:], g[key + "_tail"]), key
    assert sha(a) == str(g[key + "_sha"]), key


def _pos():
    from midastouch_amd.torch_rng import _host_state_row
    return int(_host_state_row(None).view(np.uint32)[624])


def _frame_draws(g, t, N):
    torch.manual_seed(int(g["frame_seed"]) + t)
    tn = torch.normal(mean=0.0, std=2e-4, size=(N, 3)).numpy()
    rot = torch.normal(mean=0.0, std=0.5, size=(N, 3)).numpy()
    return tn, rot


def test_oracle_loop_low_var_vs_g19_trace(golden, oracle):
    """OracleLoop (ATen's tie rule) in systematic mode, fed G19's offsets: kept sets, counts and resample indices of every frame."""
    from midastouch_amd.synthetic import make_codebook, make_trajectory
    g = golden("g19_loop_trace_low_var")
    cb = make_codebook(K=int(g["K"]), D=int(g["D"]), seed=int(g["cb_seed"]), mesh_points=20000)
    assert sha(cb.embeddings.astype(np.float32)) == str(g["cb_sha"])
    traj = make_trajectory(cb, T=int(g["T"]) + 1, seed=int(g["traj_seed"]))
    loop = oracle.OracleLoop(cb.poses, cb.embeddings, cb.mesh_vertices, ties="aten_cpu")
    poses, labels = g["poses0"], np.zeros(int(g["N0"]), dtype=np.int64)
    for t in range(1, int(g["T"]) + 1):
        N = poses.shape[0]
        assert N == int(g[f"N_{t}"]), t
        tn, rot = _frame_draws(g, t, N)
        r = loop.step(poses, labels, traj.odoms[t], traj.codes[t], tn, rot, gt=traj.gt_poses[t], mode="low_var", u32=np.float32(g[f"u32_{t}"]))
        _check_digest(g, f"nn_{t}", r["nn_idx"])
        assert r["drifted"] == bool(g[f"drifted_{t}"])
        assert r["var"] == np.float32(g[f"var_{t}"])
        _check_digest(g, f"keep_{t}", r["keep"])
        assert r["N"] == int(g[f"N2_{t}"])
        _check_digest(g, f"ridx_{t}", r["ridx"])
        poses, labels = r["poses"], r["labels"]


def test_torch_rand1_under_g19_seeds_and_word_counts(golden):
    """torch.rand(1) behind the frame's two normal draws is the stored offset, and the generator's position moves by what the draw
    sizes say: normal_words(3 N) twice from the seed (position 624: a block is due), then ONE word for the offset."""
    from midastouch_amd.torch_rng import normal_words, rand32_words
    g = golden("g19_loop_trace_low_var")
    assert rand32_words() == 1
    for t in range(1, int(g["T"]) + 1):
        N = int(g[f"N_{t}"])
        torch.manual_seed(int(g["frame_seed"]) + t)
        assert _pos() == 624
        _frame_draws(g, t, N)
        p0 = _pos()
        u = torch.rand(1)
        p1 = _pos()
        assert u.dtype == torch.float32 and np.float32(u.item()) == np.float32(g[f"u32_{t}"]), t
        assert [p0, p1] == list(g[f"pos_{t}"]), t
        words = 2 * normal_words(3 * N)
        assert p0 == (words - 1) % 624 + 1, t           # (a position of 624 means: the block is used up)
        assert p1 == (words + rand32_words() - 1) % 624 + 1, t


def _mt_from_torch():
    """numpy's MT19937 continuing torch's default CPU generator where it stands (the same recurrence; state row = block + position)."""
    from midastouch_amd.torch_rng import _host_state_row
    row = _host_state_row(None).view(np.uint32)
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": row[:624].copy(), "pos": int(row[624])}}
    return bg


def _rand32_of_word(w):
    """csrc/mt19937.hip mt_u24: the float32 value torch.rand(1) makes of one (tempered) generator output."""
    return np.float32(np.uint32(w) & np.uint32((1 << 24) - 1)) * np.float32(2.0 ** -24)


@pytest.mark.parametrize("seed", (0, 1, 42, 3001, 2**32 + 5))
def test_rand32_value_and_words_against_torch(seed):
    """The draw kind's definition against torch itself: torch.rand(1) is the low 24 bits of the NEXT generator output times 2^-24,
    and consumes exactly that one output - behind a seed, behind normal draws, behind float64 uniforms, behind another rand(1), and
    with the draw in every position around a 624-word block boundary."""
    def check(what):
        bg = _mt_from_torch()
        want = _rand32_of_word(bg.random_raw(1)[0])
        nxt = bg.random_raw(4)
        got = torch.rand(1)
        assert got.dtype == torch.float32 and np.float32(got.item()) == want, what
        assert np.array_equal(_mt_from_torch().random_raw(4), nxt), what  # one word, no more

    torch.manual_seed(seed)
    check("seed")
    torch.normal(0.0, 0.5, size=(1000, 3))
    check("normal")
    torch.rand(311, dtype=torch.float64)
    check("rand64")
    check("rand32")
    for before in (620, 621, 622, 623, 624, 625):  # the draw as word 620 .. 625 of the stream: both sides of the block boundary
        torch.manual_seed(seed)
        torch.rand(before // 2, dtype=torch.float64)
        if before % 2:
            torch.rand(1)
        check(f"word {before}")


def test_rand32_mask_is_24_bits():
    """Words whose bit 23 is set exist among the first draws: a 23-bit mask gives another value there."""
    torch.manual_seed(7)
    bg = _mt_from_torch()
    hit = 0
    for _ in range(64):
        w = np.uint32(bg.random_raw(1)[0])
        v = np.float32(torch.rand(1).item())
        assert v == _rand32_of_word(w)
        hit += v != np.float32(w & np.uint32((1 << 23) - 1)) * np.float32(2.0 ** -24)
    assert hit > 16


def test_host_bookkeeping_of_rand32():
    """torch_rng.py's host side of the draw kind: the word count, the refusal of other sizes, skip_rand32's pending skip, the scratch
    words of a counted segment, and the state hand-over - a state row stepped one word on and given back leaves torch where a host
    run stands after torch.rand(1)."""
    from midastouch_amd import _lib
    from midastouch_amd.torch_rng import (_GeneratorSide, _host_state_row, _set_host_state, counted_segment_words, normal_words,
                                          rand32_words)
    assert rand32_words(1) == 1
    with pytest.raises(_lib.MidasError):
        rand32_words(2)
    side = _GeneratorSide()
    side.pending_skip = 0
    side.skip_normal(3000).skip_rand32()
    assert side.pending_skip == normal_words(3000) + 1
    assert counted_segment_words(_lib.MT_SEGMENT_RAND32, 1, 4096) == 1
    assert counted_segment_words(_lib.MT_SEGMENT_RAND64, 1, 4096) == 8192
    assert counted_segment_words(_lib.MT_SEGMENT_NORMAL32, 3, 4096) == 3 * 4096 + 16
    for seed, before in ((3, 0), (3, 100), (4, 622), (4, 623)):  # (623: the skipped word is the block's last)
        torch.manual_seed(seed)
        torch.rand(before // 2, dtype=torch.float64) if before >= 2 else None
        if before % 2:
            torch.rand(1)
        state = torch.get_rng_state()
        torch.rand(1)
        want = torch.rand(5, dtype=torch.float64)
        torch.set_rng_state(state)
        row = _host_state_row(None).view(np.uint32).copy()
        if row[624] == 624:  # a block is due: numpy twists on the next output, as the device walk does
            bg = _mt_from_torch()
            bg.random_raw(1)
            row[:624], row[624] = bg.state["state"]["key"], bg.state["state"]["pos"]
        else:
            row[624] += 1
        _set_host_state(row, None)
        assert torch.equal(torch.rand(5, dtype=torch.float64), want), (seed, before)
