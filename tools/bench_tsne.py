#!/usr/bin/env python3
"""codebook_colors' t-SNE (midastouch_amd/tsne.py) stage by stage at K = 50 000: the embeddings route (D 256: the
t-SNE of the embeddings) and the confusion-matrix route (D 512: the K x K float64 confusion matrix, then the t-SNE of its rows,
F = K).  Stages: confusion matrix, kNN, affinities (perplexity search + joint P), PCA init, optimiser (and per iteration), total;
the kNN's dot-product rate.  --host: sklearn's TSNE(n_components=1, perplexity=40, init="pca") at K = 5000 on both routes, for the
ratio.  One JSON line.
usage: tools/bench_tsne.py [--host] [--K K] [--routes emb,confusion]"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from midastouch_amd import single_touch, tsne
from midastouch_amd.synthetic import make_codebook


def _t(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def device_route(K, D, confusion):
    E = torch.as_tensor(make_codebook("004_sugar_box", K=K, D=D, seed=1001).embeddings).to("cuda")
    res = {"K": K, "D": D, "route": "confusion" if confusion else "embeddings"}
    tsne.knn(E[:512].contiguous(), 8)  # warm-up (library, scratch)
    total = 0.0
    if confusion:
        X, t = _t(lambda: single_touch.confusion_matrix(E))
        res["confusion_s"] = t
        total += t
    else:
        X = E
    F = X.shape[1]
    k = tsne.n_neighbors(K, 40.0)
    (idx, d2), t = _t(lambda: tsne.knn(X, k, nan_to_num=confusion))
    res["knn_s"], res["knn_tflops"] = t, 2.0 * K * K * F / t / 1e12
    total += t
    (_, _, P), t = _t(lambda: tsne.affinities(idx, d2, 40.0))
    res["affinities_s"] = t
    total += t
    y0, t = _t(lambda: tsne.pca_init(X, nan_to_num=confusion))
    res["init_s"] = t
    total += t
    (y, kl, it, _), t = _t(lambda: tsne.optimize(P, y0))
    res["optimize_s"], res["n_iter"], res["kl"], res["per_iter_ms"] = t, it, kl, t / (it + 1) * 1e3
    total += t
    c, t = _t(lambda: tsne.spectral_colors(y))
    total += t
    res["total_s"] = total
    # the gradient alone (objective + raw gradient, no update)
    _, t = _t(lambda: [tsne.gradient(P, y) for _ in range(20)])
    res["gradient_ms"] = t / 20 * 1e3
    return res


def host_route(K, D, confusion):
    from sklearn.manifold import TSNE

    E = np.asarray(make_codebook("004_sugar_box", K=K, D=D, seed=1001).embeddings)
    if confusion:
        X = single_touch.confusion_matrix(torch.as_tensor(E).to("cuda")).cpu().numpy()
    else:
        X = E
    t0 = time.perf_counter()
    TSNE(n_components=1, perplexity=40, init="pca", random_state=0).fit_transform(np.nan_to_num(X))
    return {"K": K, "D": D, "route": "confusion" if confusion else "embeddings", "sklearn_s": time.perf_counter() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--K", type=int, default=50000)
    ap.add_argument("--routes", default="emb,confusion")
    a = ap.parse_args()
    out = {"device": []}
    for r in a.routes.split(","):
        conf = r == "confusion"
        out["device"].append(device_route(a.K, 512 if conf else 256, conf))
        torch.cuda.empty_cache()
    if a.host:
        out["host"] = [host_route(5000, 512 if r == "confusion" else 256, r == "confusion") for r in a.routes.split(",")]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
