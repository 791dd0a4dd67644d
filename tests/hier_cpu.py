"""A model without a GPU for the host route of ``LatentIndex.hierarchy``: ``peaks_cpu``'s engine, which keeps an index's rows in host
memory and answers create, add, read, names and the exact search; the device's spanning tree is not there: asking for it is an error, so
a test that passes ran the twin."""
import peaks_cpu


class RowsEngine(peaks_cpu.RowsEngine):
    def index_mst(self, ix, core2=None):
        raise AssertionError("the device's spanning tree was asked of a model without a GPU")


class RowsModel(peaks_cpu.RowsModel):
    def __init__(self, dense_out=4, global_dim=9):
        super().__init__(dense_out, global_dim)
        self.engine = RowsEngine()
