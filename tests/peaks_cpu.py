"""A model without a GPU for the host route of ``LatentIndex.density_peaks``: an engine that keeps an index's rows in host memory and
answers what the host route asks of it -- create, add, read, names and the exact search (the twin's distances under the search's total
order).  The device passes are not there: asking for them is an error, so a test that passes ran the twins."""
import numpy as np

from scann import _hip


class _Rows:
    def __init__(self, dim):
        self.dim = int(dim)
        self.rows = np.zeros((0, self.dim), np.float32)
        self.ids = np.zeros(0, np.int64)
        self.atoms = np.zeros(0, np.int32)

    def __len__(self):
        return len(self.rows)

    def free(self):
        pass


class RowsEngine:
    def index_create(self, dim):
        return _Rows(dim)

    def index_add(self, ix, rows, ids=None, atoms=None):
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, ix.dim)
        n = len(rows)
        ix.ids = np.concatenate([ix.ids, np.arange(len(ix), len(ix) + n) if ids is None else np.asarray(ids, np.int64)])
        ix.atoms = np.concatenate([ix.atoms, np.full(n, -1, np.int32) if atoms is None else np.asarray(atoms, np.int32)])
        ix.rows = np.concatenate([ix.rows, rows])

    def index_read(self, ix, first=0, n=None):
        n = len(ix) - first if n is None else n
        return ix.rows[first:first + n].copy(), ix.ids[first:first + n].copy(), ix.atoms[first:first + n].copy()

    def index_names(self, ix):
        return ix.ids.copy(), ix.atoms.copy()

    def index_query(self, ix, q, k, query_ids=None):
        d = _hip.knn_dist2_matrix(q, ix.rows)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # (stable: equal distances stay in position order)
        return {"dist2": np.take_along_axis(d, order, axis=1), "position": order.astype(np.int32), "id": ix.ids[order], "atom": ix.atoms[order]}

    def index_peaks(self, ix, gamma):
        raise AssertionError("the device passes were asked of a model without a GPU")


class RowsModel:
    def __init__(self, dense_out=4, global_dim=9):
        self.config = {"model": {"dense_out": dense_out, "global_dim": global_dim}}
        self.engine = RowsEngine()
