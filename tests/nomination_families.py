"""The kernel families of K3 as the nomination hooks reach them (TEST INFRASTRUCTURE, shared by tests/test_gpu_nominations.py and
tests/test_gpu_level_stage.py): per family the tuning keys that force it, and a wrapper that runs a hook call and ASSERTS the route it
took."""
import numpy as np

from tests import nominate_ref as ref

ROWREG, LDSROW, LEVEL = 0, 1, 2
ARITH_CODE = {"bf16x3": 0, "f16x2": 1, "f16x1": 2, "f32": 3}
RESTORE = dict(gemm_bf16x3=1, gemm_rowreg=1, gemm_nominate=0, gemm_image=1, gemm_ldsrow=1, gemm_qsplit=1, gemm_blocks=0)

# name -> (tuning keys, family, arithmetic, from the image, query counts per call the variant allows)
FAMILIES = {
    "rowreg-bf16x3": (dict(gemm_nominate=1, gemm_image=0), ROWREG, "bf16x3", False, (1, 64)),
    "rowreg-f16x2-rows": (dict(gemm_nominate=2, gemm_image=0), ROWREG, "f16x2", False, (1, 64)),
    "rowreg-f16x2-image": (dict(gemm_nominate=2, gemm_image=1), ROWREG, "f16x2", True, (1, 64)),
    "rowreg-f16x1-rows": (dict(gemm_nominate=3, gemm_image=0), ROWREG, "f16x1", False, (1, 64)),
    "rowreg-f16x1-image": (dict(gemm_nominate=3, gemm_image=1), ROWREG, "f16x1", True, (1, 64)),
    "ldsrow-bf16-nqt1": (dict(gemm_rowreg=0), LDSROW, "bf16x3", False, (1, 32)),
    "ldsrow-bf16-nqt2": (dict(gemm_rowreg=0), LDSROW, "bf16x3", False, (33, 64)),
    "ldsrow-f32-nqt1": (dict(gemm_bf16x3=0), LDSROW, "f32", False, (1, 32)),
    "ldsrow-f32-nqt2": (dict(gemm_bf16x3=0), LDSROW, "f32", False, (33, 64)),
    "level-bf16": (dict(gemm_rowreg=0, gemm_ldsrow=0), LEVEL, "bf16x3", False, (1, 64)),
    "level-f32": (dict(gemm_bf16x3=0, gemm_ldsrow=0), LEVEL, "f32", False, (1, 64)),
}
ROWREG_FAMILIES = [n for n, f in FAMILIES.items() if f[1] == ROWREG]


class Family:
    def __init__(self, name, ctx):
        self.name = name
        self.keys, self.family, self.arith, self.image, (self.nq_min, self.nq_max) = FAMILIES[name]
        self.bound = ref.F32_ERR[self.arith]
        self.ctx = ctx

    def corpus(self, rows):
        import semtools_amd as smt

        c = smt.Corpus(self.ctx)
        c.append(rows)
        if self.image:
            c.prepack(True)
        return c

    def route(self, filtered=False, family=None):
        return (self.family if family is None else family) | (ARITH_CODE[self.arith] << 4) | (0x100 if self.image else 0) | (0x200 if filtered else 0)

    def run(self, c, qs, tau=None, buffered=False, ranges=None, route=None, level=None):
        """One hook call; the route it took must be the family's."""
        assert self.nq_min <= len(qs) <= self.nq_max, (self.name, len(qs))
        dist, hits, counts, got_route = c.debug_nominations(qs, tau=tau, buffered=buffered, ranges=ranges, level=level)
        want = self.route(ranges is not None) if route is None else route
        assert got_route == want, f"{self.name}: route {got_route:#x}, expected {want:#x}"
        return dist, hits, counts

    def run_all(self, c, qs):
        """All-pass nominations of any number of queries, in calls of a size the variant allows (the last call is topped up from
        the front).  Checks that nothing is missing or doubled on the way.  Returns dist [rows][len(qs)]."""
        out = np.empty((c.rows, len(qs)), dtype=np.float32)
        step = self.nq_max
        for q0 in range(0, len(qs), step):
            idx = list(range(q0, min(q0 + step, len(qs))))
            idx += list(range(0, max(0, self.nq_min - len(idx))))
            dist, hits, counts = self.run(c, qs[idx])
            assert np.all(hits == 1) and not np.isnan(dist).any(), self.name
            assert np.all(counts[:len(idx)] == c.rows) and np.all(counts[len(idx):] == 0), (self.name, counts)
            n_own = min(step, len(qs) - q0)
            out[:, q0:q0 + n_own] = dist[:, :n_own]
        return out

    def bootstrap(self, c, qs, ranges=None):
        """The bootstrap launch of the call (smt_debug_bootstrap_minima); the route must be the family's.  -> (tile_min, stride)"""
        tile_min, stride, got_route = c.debug_bootstrap_minima(qs, ranges=ranges)
        assert got_route == self.route(ranges is not None), f"{self.name}: route {got_route:#x}"
        return tile_min, stride


def set_family(ctx, f):
    for k, v in {**RESTORE, **f.keys}.items():
        ctx.set_tuning(k, v)


def restore(ctx):
    for k, v in RESTORE.items():
        ctx.set_tuning(k, v)
