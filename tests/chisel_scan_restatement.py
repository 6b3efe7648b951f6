"""CPU restatement of open_chisel's projective depth + colour scan integrate, for the tests (not product code):
Chisel::IntegrateDepthScanColorWithOneCameraModelBGR (Chisel.h:198-258) with
ProjectionIntegrator::IntegrateColorWithOneCameraModelBGR (ProjectionIntegrator.h:189-269), the frustum of
PinholeCamera::SetupFrustum (PinholeCamera.cpp:55-59 -> Frustum.cpp:150-196, :100-125) and the chunk list of
ChunkManager::GetChunkIDsIntersecting (ChunkManager.cpp:241-271, Frustum::Intersects Frustum.cpp:41-79).

numpy, every operation in np.float32 in the reference's order (3-term sums are a0 + (a1 + a2), as the project assumes
for Eigen 3.3), one scan vectorised over the listed chunks.  tests/test_chisel_scan_reference.py pins it against maps the
reference itself built (tests/golden/chisel_scan_reference_*); the GPU tests then lean on it at sizes the goldens do not
hold.  The chunk container's iteration order is not restated.

The map lives in a `store`: anything with get(id) -> (sdf, weight, kfid, rgbw) or None, and set(id, planes).  DictStore
is the plain one; tests put an oracle chisel map behind the same two calls to mix scans with InsertCloud key frames."""
import math

import numpy as np

F = np.float32
TRUNC = (0.0019, -0.00152, 0.001504, 6.0)      # ChiselServer.cpp:56-59


# per-scan counters of the depth classes and voxel states a scan met (tests/chisel_scan_edge_scenario.py asserts on them):
#   int_*   voxels INTEGRATED through a pixel of that class        on_*  voxels that project onto a pixel of that class
#   cand_*  carving candidates (surfaceDist > truncation + carvingDist) by the state the voxel was in; *_reset of them reset
CLASS_COUNTERS = ("int_pos_zero", "int_neg_zero", "int_negative", "int_tiny", "int_far", "int_pos_inf", "int_neg_inf",
                  "on_pos_inf", "on_neg_inf", "on_nan", "on_negative", "int_cw4", "int_cw5", "int_cw255", "int_w_negative",
                  "int_w_huge", "cand_sdf_f32_1e5", "cand_sdf_f32_1e5_reset", "cand_sdf_above_1e5", "cand_sdf_above_1e5_reset",
                  "cand_sdf_below_1e5_reset", "cand_w_neg_zero", "cand_w_subnormal_reset", "cand_w_negative",
                  "cand_w_tiny_reset")
SDF_EDGE = np.float32(1e-5)                    # below the double 1e-5 the reference compares with


def s3(a, b, c):
    return a + (b + c)


class DictStore:
    def __init__(self):
        self.chunks = {}

    def get(self, *cid):                       # get((x, y, z)) or get(x, y, z)
        return self.chunks.get(tuple(int(v) for v in (cid[0] if len(cid) == 1 else cid)))

    def set(self, cid, planes):
        self.chunks[cid] = planes

    def ids(self):
        return sorted(self.chunks)


def fresh_planes(n=1):
    return (np.full((n, 4096), 99999.0, F), np.zeros((n, 4096), F), np.zeros((n, 4096), np.uint32),
            np.zeros((n, 4096), np.uint32))


class ScanIntegrator:
    def __init__(self, resolution, cam, near, far, carving=False, carving_dist=0.05, trunc=TRUNC, weight=1.0, store=None):
        self.res = F(resolution)
        self.cam = cam
        self.near, self.far = F(near), F(far)
        self.carving, self.carving_dist = bool(carving), F(carving_dist)
        self.tq, self.tl, self.tc, self.ts = (F(v) for v in trunc)
        self.weight = F(weight)
        self.half = self.res * F(0.5)                                   # ChunkManager.cpp:68
        self.rounding = F(1.0) / (F(16) * self.res)                     # ChunkManager.cpp:91
        self.diag = F(2.0 * math.sqrt(float(F(3.0))) * float(self.res))  # formed in double, stored as float
        self.store = store if store is not None else DictStore()

    # ---- frustum and chunk list
    def frustum(self, Twc):
        c = self.cam
        Twc = np.asarray(Twc, F).reshape(3, 4)
        R, t = Twc[:, :3], Twc[:, 3]
        right, up, fwd = R[:, 0], -R[:, 1], R[:, 2]
        fy, cy, width, height = F(c["fy"]), F(c["cy"]), F(c["width"]), F(c["height"])
        fx = fy                                                         # SetupFrustum hands fy over twice
        aspect = (fx * width) / (fy * height)
        fov = F(math.atan2(float(cy), float(fy)) + math.atan2(float(height - cy), float(fy)))
        tang = F(math.tan(float(fov / F(2))))
        hf = tang * self.far
        wf = hf * aspect
        hn = tang * self.near
        wn = hn * aspect
        fc, nc = t + fwd * self.far, t + fwd * self.near
        ftl = fc + (up * hf) - (right * wf)
        ftr = fc + (up * hf) + (right * wf)
        fbl = fc - (up * hf) - (right * wf)
        fbr = fc - (up * hf) + (right * wf)
        ntl = nc + (up * hn) - (right * wn)
        ntr = nc + (up * hn) + (right * wn)
        nbl = nc - (up * hn) - (right * wn)
        nbr = nc - (up * hn) + (right * wn)

        def plane(a, b, cc):
            ab, ac = b - a, cc - a
            cr = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]], F)
            z = s3(cr[0] * cr[0], cr[1] * cr[1], cr[2] * cr[2])
            n = cr / np.sqrt(z) if z > 0 else cr
            return n.astype(F), -s3(cr[0] * a[0], cr[1] * a[1], cr[2] * a[2])   # the distance of the unnormalised normal

        planes = [plane(ftr, ftl, fbr), plane(nbl, ntl, nbr), plane(ntl, ftl, ntr), plane(nbr, fbl, nbl),
                  plane(ftl, ntl, fbl), plane(ntr, ftr, nbr)]              # far, near, top, bottom, left, right
        corners = np.stack([ftl, ftr, fbl, fbr, nbr, ntl, ntr, nbl])
        lo = np.floor(corners.min(0) * self.rounding).astype(np.int64) - 1
        hi = np.floor(corners.max(0) * self.rounding).astype(np.int64) + 2
        return np.stack([p[0] for p in planes]), np.array([p[1] for p in planes], F), lo, hi

    def chunk_list(self, Twc):
        """[n, 3] int32 ids in the reference's list order (x outermost)."""
        n, d, lo, hi = self.frustum(Twc)
        g = np.stack(np.meshgrid(*[np.arange(lo[k], hi[k] + 1) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
        bmin = (g * 16).astype(F) * self.res
        ext = F(16.0) * self.res
        hit = np.zeros(len(g), bool)
        for p in range(6):
            v = np.where(n[p][None, :] < 0, bmin, bmin + ext)
            hit |= s3(v[:, 0] * n[p, 0], v[:, 1] * n[p, 1], v[:, 2] * n[p, 2]) + d[p] > 0
        return g[hit].astype(np.int32)

    @staticmethod
    def _count_classes(st, on, d, m1, m2, mr, sdf, w, cw):
        neg0 = (d == 0) & np.signbit(d)
        with np.errstate(all="ignore"):
            cls = dict(pos_zero=(d == 0) & ~neg0, neg_zero=neg0, negative=d < 0, tiny=(d > 0) & (d < F(1e-3)), far=d == F(25.0),
                       pos_inf=d == F(np.inf), neg_inf=d == F(-np.inf))
            for k, m in cls.items():
                st["int_" + k] += int((m1 & m).sum())
            for k in ("pos_inf", "neg_inf", "negative"):
                st["on_" + k] += int((on & cls[k]).sum())
            st["on_nan"] += int((on & np.isnan(d)).sum())
            for k, m in (("cw4", cw == 4), ("cw5", cw == 5), ("cw255", cw == 255), ("w_negative", w < 0), ("w_huge", w > F(1e29))):
                st["int_" + k] += int((m1 & m).sum())
            up = np.nextafter(SDF_EDGE, F(1))
            tiny = np.finfo(F).tiny
            for k, m in (("sdf_f32_1e5", sdf == SDF_EDGE), ("sdf_above_1e5", sdf == up)):
                st["cand_" + k] += int((m2 & (w > 0) & m).sum())
                st["cand_" + k + "_reset"] += int((mr & m).sum())
            st["cand_sdf_below_1e5_reset"] += int((mr & (sdf == np.nextafter(SDF_EDGE, F(0)))).sum())
            st["cand_w_neg_zero"] += int((m2 & (w == 0) & np.signbit(w)).sum())
            st["cand_w_negative"] += int((m2 & (w < 0)).sum())
            st["cand_w_subnormal_reset"] += int((mr & (w > 0) & (w < tiny)).sum())
            st["cand_w_tiny_reset"] += int((mr & (w >= tiny) & (w < F(1e-14))).sum())

    # ---- one scan
    def integrate_scan(self, depth, bgr, Twc, slab=256):
        """-> dict(listed, created, kept, collected, integrated, reset, visits, updated [ids])"""
        c = self.cam
        depth = np.ascontiguousarray(depth, F)
        bgr = np.ascontiguousarray(bgr, np.uint8)
        assert depth.shape == (c["height"], c["width"]) and bgr.shape[:2] == depth.shape and bgr.shape[2] in (3, 4)
        Twc = np.asarray(Twc, F).reshape(3, 4)
        ids = self.chunk_list(Twc)
        st = dict(listed=len(ids), created=0, kept=0, collected=0, integrated=0, reset=0, visits=0, updated=[], zero_depth=0,
                  **{k: 0 for k in CLASS_COUNTERS})
        for a in range(0, len(ids), slab):
            self._slab(ids[a:a + slab], depth.reshape(-1), bgr.reshape(-1, bgr.shape[2]), Twc, st)
        st["collected"] = st["created"] - st["kept"]
        st["visits"] = st["integrated"] + st["reset"]
        return st

    def _slab(self, ids, depth, bgr, Twc, st):
        c = self.cam
        L = len(ids)
        R, t = Twc[:, :3], Twc[:, 3]
        fx, fy, cx, cy = F(c["fx"]), F(c["fy"]), F(c["cx"]), F(c["cy"])
        width, height = F(c["width"]), F(c["height"])
        loc = np.arange(16).astype(F) * self.res + self.half              # centroids (ChunkManager.cpp:60-75)
        org = (ids * 16).astype(F) * self.res                             # Chunk origin
        cen = [loc[None, :] + org[:, k:k + 1] for k in range(3)]          # [L, 16] per axis
        dx = (cen[0] - t[0])[:, None, None, :]
        dy = (cen[1] - t[1])[:, None, :, None]
        dz = (cen[2] - t[2])[:, :, None, None]
        with np.errstate(all="ignore"):
            p = [s3(R[0, q] * dx, R[1, q] * dy, R[2, q] * dz).reshape(L, 4096) for q in range(3)]   # R^T (c - t)
            inv_z = F(1.0) / p[2]
            u = fx * p[0] * inv_z + cx
            v = fy * p[1] * inv_z + cy
            on = (u >= 0) & (v >= 0) & (u < width) & (v < height) & ~(p[2] < 0)
            pix = np.where(on, v.astype(np.int64) * c["width"] + u.astype(np.int64), 0)
            d = depth[pix]
            ok = on & ~np.isnan(d)
            tau = (self.tq * d * d + self.tl * d + self.tc) * self.ts      # not floored here
            s = d - p[2]
            m1 = ok & (np.abs(s) < tau + self.diag)
            m2 = ok & ~m1 & (s > tau + self.carving_dist) if self.carving else np.zeros_like(m1)
            have = [self.store.get(tuple(int(x) for x in cid)) for cid in ids]
            sdf, w, kf, col = fresh_planes(L)
            for i, pl in enumerate(have):
                if pl is not None:
                    sdf[i], w[i], kf[i], col[i] = pl
            sdf0, w0 = sdf.copy(), w.copy()
            # colour (ColorVoxel::IntegrateSimple through ColorImage::AtBGR), only while the colour weight is below 5
            cw = col >> 24
            mc = m1 & (cw < 5)
            px = bgr[pix]
            inv = F(1.0) / (1 + cw).astype(F)
            new = [((cw * ((col >> sh) & 255) + px[..., ch]).astype(F) * inv).astype(np.uint8).astype(np.uint32)
                   for sh, ch in ((0, 2), (8, 1), (16, 0))]
            col = np.where(mc, new[0] | (new[1] << 8) | (new[2] << 16) | ((cw + 1) << 24), col).astype(np.uint32)
            # DistVoxel::Integrate(s, weight / (2 tau))
            wu = self.weight / (F(2.0) * tau)
            nsdf = (w * sdf + wu * s) / (wu + w)
            nw = w + wu
            # Reset (carving)
            mr = m2 & (w > 0) & (sdf.astype(np.float64) < 1e-5)
            sdf = np.where(m1, nsdf, np.where(mr, F(99999.0), sdf)).astype(F)
            w = np.where(m1, nw, np.where(mr, F(0), w)).astype(F)
            kf = np.where(mr, np.uint32(0), kf).astype(np.uint32)
        st["integrated"] += int(m1.sum())
        st["reset"] += int(mr.sum())
        st["zero_depth"] += int((m1 & (d == 0)).sum())
        self._count_classes(st, on, d, m1, m2, mr, sdf0, w0, cw)
        upd = (m1 | mr).any(1)
        for i, cid in enumerate(ids):
            key = tuple(int(x) for x in cid)
            if have[i] is None:
                st["created"] += 1
                if not upd[i]:
                    continue                                            # created, not updated: garbage-collected
                st["kept"] += 1
            if upd[i]:
                st["updated"].append(key)
                self.store.set(key, (sdf[i].copy(), w[i].copy(), kf[i].copy(), col[i].copy()))
