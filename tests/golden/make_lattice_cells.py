"""Writes tests/golden/lattice_cells.npz: the neighbour lists scann.utils.voronoi_neighbor.compute_voronoi_neighbor(struct, 7, 4.0, 0.2)
gives for seven small unit cells -- the commonest kind of entry of an MP2018-style set.  A primitive cell's Voronoi facets belong to
periodic images of its own few sites, so these lists are multigraphs with self-loops: fcc Cu lists atom 0 twelve times as the
neighbour of atom 0.  Plain arrays only (per structure: Z, CSR offsets, neighbour index, solid angle, ratio, distance), needs SciPy:

    python tests/golden/make_lattice_cells.py

tests/test_crystal_host.py regenerates the lists (where SciPy is present) and compares them with the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "scann--material_amd"))

CUTOFF, D_THRESH, W_THRESH = 7, 4.0, 0.2
NAMES = ("fcc_Cu", "bcc_Fe", "hcp_Mg", "NaCl", "diamond_C", "CsCl", "SrTiO3")

FCC = 0.5 * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], float)
BCC = 0.5 * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]], float)


def structures():
    """name -> (lattice rows [A], symbols, fractional coordinates); experimental lattice constants at room temperature"""
    a_mg, c_mg = 3.209, 5.211
    hexagonal = np.array([[a_mg, 0, 0], [-0.5 * a_mg, 0.5 * np.sqrt(3) * a_mg, 0], [0, 0, c_mg]])
    return {
        "fcc_Cu": (3.615 * FCC, ["Cu"], [[0, 0, 0]]),
        "bcc_Fe": (2.866 * BCC, ["Fe"], [[0, 0, 0]]),
        "hcp_Mg": (hexagonal, ["Mg", "Mg"], [[1 / 3, 2 / 3, 0.25], [2 / 3, 1 / 3, 0.75]]),
        "NaCl": (5.640 * FCC, ["Na", "Cl"], [[0, 0, 0], [0.5, 0.5, 0.5]]),
        "diamond_C": (3.567 * FCC, ["C", "C"], [[0, 0, 0], [0.25, 0.25, 0.25]]),
        "CsCl": (4.123 * np.eye(3), ["Cs", "Cl"], [[0, 0, 0], [0.5, 0.5, 0.5]]),
        "SrTiO3": (3.905 * np.eye(3), ["Sr", "Ti", "O", "O", "O"],
                   [[0, 0, 0], [0.5, 0.5, 0.5], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]]),
    }


def neighbour_arrays():
    """name -> dict(Z, offset, index, angle, ratio, distance) from our own Voronoi builder"""
    from scann.utils import voronoi_neighbor as vn

    out = {}
    for name, (lattice, species, frac) in structures().items():
        s = vn.Structure(lattice, species, frac, coords_are_cartesian=False)
        lists = vn.compute_voronoi_neighbor(s, CUTOFF, D_THRESH, W_THRESH)
        assert len(lists) == len(s)
        flat = [e for lst in lists for e in lst]
        out[name] = dict(Z=np.asarray(s.atomic_numbers, np.int32),
                         offset=np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).astype(np.int32),
                         index=np.asarray([e[1] for e in flat], np.int32),
                         angle=np.asarray([e[2] for e in flat], np.float64),
                         ratio=np.asarray([e[3] for e in flat], np.float64),
                         distance=np.asarray([e[4] for e in flat], np.float64))
    return out


if __name__ == "__main__":
    arrays = {"%s/%s" % (name, k): v for name, d in neighbour_arrays().items() for k, v in d.items()}
    np.savez_compressed(os.path.join(HERE, "lattice_cells.npz"), **arrays)
    for name, d in neighbour_arrays().items():
        deg = np.diff(d["offset"])
        own = sum(int((d["index"][d["offset"][a]:d["offset"][a + 1]] == a).sum()) for a in range(len(deg)))
        distinct = [len(set(d["index"][d["offset"][a]:d["offset"][a + 1]].tolist())) for a in range(len(deg))]
        print("%-10s atoms %d  edges per atom %s  to the atom itself %d  distinct neighbours %s" % (name, len(deg), deg.tolist(), own, distinct))
