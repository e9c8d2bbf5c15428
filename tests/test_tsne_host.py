"""Host-side checks of midastouch_amd/tsne.py: the argument rules of sklearn's TSNE, the refusal of CPU tensors, and the
init="random" draw (no GPU needed)."""
import numpy as np
import pytest
import torch


def test_neighbour_count_and_perplexity_rules():
    from midastouch_amd import tsne
    from midastouch_amd.ops import MidasError

    assert tsne.n_neighbors(50000, 40.0) == 121
    assert tsne.n_neighbors(50, 40.0) == 49
    assert tsne.n_neighbors(3, 1.0) == 2
    for K, perp in ((40, 40.0), (100, 0.0), (100, -1.0)):
        with pytest.raises(MidasError):
            tsne.n_neighbors(K, perp)
    with pytest.raises(MidasError):
        tsne.n_neighbors(5000, 90.0)  # 271 neighbours


def test_cpu_tensors_and_bad_shapes_are_refused():
    from midastouch_amd import single_touch, tsne
    from midastouch_amd.ops import MidasError

    X = torch.zeros((100, 8))
    for fn in (lambda: tsne.tsne_1d(X), lambda: tsne.knn(X, 5), lambda: single_touch.color_tsne(X),
               lambda: single_touch.codebook_colors(X), lambda: tsne.pca_init(X)):
        with pytest.raises(MidasError):
            fn()


def test_random_init_is_sklearns_draw():
    sk = pytest.importorskip("sklearn.utils")
    from midastouch_amd import tsne

    ref = 1e-4 * sk.check_random_state(0).standard_normal(size=(1000, 1)).astype(np.float32)
    got = tsne.random_init(1000, 0).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.reshape(-1).view(np.uint32))
