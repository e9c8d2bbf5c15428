"""The oracle-backed shard backend (tests/_oracle_shard_backend.py) with the frame's pose estimate (TESTS ONLY), in numpy
float64: per 256-particle block the partial sums of the moments, gathered in rank order, added one block after the other and
closed as oracle.cluster_centers closes a cluster (float32 weights, the isclose flatten rule, eigh of the moment matrix,
spread about the float32 centre).  The partial layout is this backend's own (the engine treats it as opaque)."""
import numpy as np
import torch
from scipy.spatial.transform import Rotation

from tests._oracle_shard_backend import OracleShardBackend

EST_BLOCK = 256
# one block: sum w | count | max w | min w | sum w q q^T (16) | sum q q^T (16) | sum w t | sum t | sum w t^2 | sum t^2 (3 each)
O_SW, O_CNT, O_MAX, O_MIN, O_QQW, O_QQ1, O_TW, O_T1, O_TTW, O_TT1, O_MOM = 0, 1, 2, 3, 4, 20, 36, 39, 42, 45, 48


class OracleEstimateBackend(OracleShardBackend):
    def estimate_alloc(self, st, world):
        st.est_part = torch.zeros(-(-st.N // EST_BLOCK) * O_MOM, dtype=torch.float64)
        st.est_center = torch.zeros((4, 4), dtype=torch.float32)
        st.est_stds = torch.zeros((3,), dtype=torch.float32)

    def estimate_moments(self, st):
        P = st.poses_prop.numpy().astype(np.float64)
        w = st.weights.numpy().astype(np.float32).astype(np.float64)  # particles.weights.float()
        q = Rotation.from_matrix(P[:, :3, :3]).as_quat()  # x, y, z, w
        q[q[:, 3] < 0] *= -1.0
        t = P[:, :3, 3]
        part = st.est_part.numpy().reshape(-1, O_MOM)
        for b in range(part.shape[0]):
            sl = slice(b * EST_BLOCK, min((b + 1) * EST_BLOCK, st.N))
            wb, qb, tb = w[sl], q[sl], t[sl]
            row = part[b]
            row[O_SW], row[O_CNT], row[O_MAX], row[O_MIN] = wb.sum(), float(len(wb)), wb.max(), wb.min()
            row[O_QQW:O_QQW + 16] = np.einsum("n,ni,nj->ij", wb, qb, qb).ravel()
            row[O_QQ1:O_QQ1 + 16] = np.einsum("ni,nj->ij", qb, qb).ravel()
            row[O_TW:O_TW + 3], row[O_T1:O_T1 + 3] = (tb * wb[:, None]).sum(axis=0), tb.sum(axis=0)
            row[O_TTW:O_TTW + 3], row[O_TT1:O_TT1 + 3] = (tb * tb * wb[:, None]).sum(axis=0), (tb * tb).sum(axis=0)
        return st.est_part

    def estimate_finish(self, st, part_all, world):
        part = part_all.numpy().reshape(-1, O_MOM)
        acc = part[0].copy()
        for b in range(1, part.shape[0]):  # block after block, in rank order
            acc = acc + part[b]
        mx, mn = part[:, O_MAX].max(), part[:, O_MIN].min()
        flat = abs(np.float32(np.float32(mx) - np.float32(mn))) <= 1e-8  # isclose(max - min, 0): every weight 1
        sw = acc[O_CNT] if flat else acc[O_SW]
        M = acc[O_QQ1:O_QQ1 + 16] if flat else acc[O_QQW:O_QQW + 16]
        tw = acc[O_T1:O_T1 + 3] if flat else acc[O_TW:O_TW + 3]
        ttw = acc[O_TT1:O_TT1 + 3] if flat else acc[O_TTW:O_TTW + 3]
        evals, evecs = np.linalg.eigh(M.reshape(4, 4) / sw)
        aq = evecs[:, np.argmax(evals)]
        if aq[3] < 0:
            aq = -aq
        c = np.zeros((4, 4), dtype=np.float32)
        c[:3, :3] = Rotation.from_quat(aq).as_matrix()
        c[:3, 3] = tw / sw
        c[3, 3] = 1.0
        m = c[:3, 3].astype(np.float64)
        var = np.maximum((ttw - 2.0 * m * tw + m * m * sw) / sw, 0.0)
        st.est_center.copy_(torch.as_tensor(c))
        st.est_stds.copy_(torch.as_tensor(np.sqrt(var).astype(np.float32)))
