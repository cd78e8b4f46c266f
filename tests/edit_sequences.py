"""Shared driver of the edit-sequence tests (test_edit_sequences_cpu.py, test_gpu_edit_sequences.py): seeded random and scripted ORDERS of
the scene edits — append (both placement modes), removal, regraft, geometry edits by all four calls, material and texture edits, the cost
readout — with frames, ray queries and denoiser probes in between, on one live context.  The single-feature tests start nearly every case
from a fresh upload; the edits share state that outlives a call (exact node boxes, parent links, the host's vertex and topology copies,
the level grouping, array capacities, the compacted object-space copy, the placement mode, denoiser flags), and a stale flag shows only
when one specific edit follows another.
The Python `Scene` of the mirror is the only source of truth for what the scene is.  After every op the context is held against the
rule the header states for that edit (check_graft, check_placed_graft, check_prune, expected_dirty_nodes, tree_cost_ref), the invariants
of the tree, a fresh context that uploads the mirror's scene (lights, emissive list), a brute force over the scene's own triangles (ray
queries: hit distance bit for bit) and, for frames, the oracle walking the exported tree (bit for bit).  Every comparison is exact but
the cost sums (regraft_common.COST_RTOL).
The ops of a sequence are drawn from np.random.default_rng([BASE, seed]) and depend on the mirror's scene only (mesh and material
counts), never on anything the context returns: one seed is one op list on host-only contexts, on the device and under every builder.
A helper, not a test file."""
import re
from collections import Counter
from dataclasses import replace

import numpy as np

import bruteforce
import placement_ref as pr
import regraft_common as rc
from append_common import PLACE, add_emitter_material, append_patch, check_graft
from common import SCENES, bits_equal, check_bvh_invariants, struct_equal
from fypraytracer_amd import capi
from partial_refit_common import expected_dirty_nodes, mesh_triangles
from remove_common import BRANCHES, check_prune, removed_triangles

BASE = 20261                               # first word of every sequence's seed
W, H = 64, 48                              # frames of the sequences
SIZES = (1, 4, 5, 65, 300)                 # a leaf code | a full leaf | the device builders' threshold | two workgroups' worth | several levels
TOPOLOGY = ("append m0", "append m1", "remove", "regraft")
FOLLOWERS = TOPOLOGY + ("partial move", "full move")
MOVE_CALLS = ("update_mesh_vertices", "update_transforms key 22 = 0", "update_transforms key 22 = 1", "update_vertices")
TECHS = (capi.RESTIR_DI, capi.RESTIR_GI, capi.NEE, capi.BRDF_SAMPLING)
ESTATE = -3
# op weights: a frame about every third op (never below one per four others)
WEIGHTS_HOST = dict(append=4, remove=3, regraft=3, material=2, texture=1, mode=2, cost=1)
WEIGHTS_DEVICE = dict(append=4, remove=3, regraft=3, move=5, material=2, texture=2, mode=2, cost=2, frame=11, denoise=3)


def same_exports(a, b, n_meshes):
    """Light trees and emissive list of two contexts, bit for bit."""
    la, lb = a.export_lighttrees(n_meshes), b.export_lighttrees(n_meshes)
    for k in ("tlas", "blas"):
        assert len(la[k]) == len(lb[k]) and struct_equal(la[k], lb[k]).all(), k
    assert la["tlas_root"] == lb["tlas_root"]
    for k in ("blas_first", "blas_count", "blas_root"):
        assert np.array_equal(la[k], lb[k]), k
    assert np.array_equal(a.export_emissive(), b.export_emissive())


def _scene_bvh(sc):
    """Leaf records straight from the scene's world vertices (what the device must hold after an edit), in export_bvh's shape."""
    pos = sc.world_vertices["position"].astype(np.float32)
    t = sc.triangles
    tris = np.zeros(len(t), dtype=capi.BVH_TRI_DTYPE)
    tris["v0"], tris["e1"], tris["e2"] = pos[t["v0"]], pos[t["v1"]] - pos[t["v0"]], pos[t["v2"]] - pos[t["v0"]]
    tris["tri"] = np.arange(len(t), dtype=np.uint32)
    return {"tris": tris}


class Ledger:
    """What the sequences of one test file met (its coverage test reads it last)."""

    def __init__(self):
        self.ops = Counter()
        self.pairs, self.kinds, self.branches, self.partial = set(), set(), set(), set()
        self.emptied = self.leaf_root = self.grew = False

    def missing(self, device):
        """The conditions of the coverage test that do not hold, as text (empty: all hold)."""
        kinds = ("append", "remove", "regraft", "material", "texture", "mode", "cost") + (("move", "frame", "denoise") if device else ())
        out = [f"op {k} met {self.ops[k]} times (< 10)" for k in kinds if self.ops[k] < 10]
        followers = FOLLOWERS if device else TOPOLOGY
        out += [f"pair {a} -> {b} not met" for a in TOPOLOGY for b in followers if (a, b) not in self.pairs]
        out += [f"placement kind {k} not met" for k in (pr.FIRST, pr.SLOT, pr.PAIR, pr.ROOT_PAIR) if k not in self.kinds]
        # (the host builder makes one sub-tree per mesh: no leaf of a host-built tree holds triangles of two meshes, so "leaf partly
        # emptied" is the device builders' to meet, as in test_remove_cpu.py / test_gpu_remove.py)
        out += [f"prune branch '{b}' not met" for b in (BRANCHES if device else BRANCHES[1:]) if b not in self.branches]
        out += [what for what, met in (("an emptied tree", self.emptied), ("a leaf-code root", self.leaf_root)) if not met]
        if device:
            out += [] if self.grew else ["capacity growth not met"]
            out += [f"partial = {p} not met" for p in (0, 1) if p not in self.partial]
        return out


def _error_code(e):
    return int(re.search(r"fyprt error (-?\d+)", str(e)).group(1))


def _state(call):
    """What a readout returns, or the error code it answers (compared before and after an edit that must not touch it)."""
    try:
        r = call()
    except capi.FyprtError as e:
        return ("error", _error_code(e))
    return tuple(int(getattr(r, f)) for f, _ in r._fields_)


class EditMirror:
    """A context (`device` = -1: host-only, else the GPU), the Python scene it must equal, and the flags the header lets a caller rely on.
    `ops`: a scripted op list, or None for `n_ops` random ones.  `geometry_ops`: the generator draws moves, frames and denoiser probes
    (device contexts only: host-only contexts refuse the geometry calls).  `object_copy`: the context holds the object-space copy
    (fyprt_set_object_vertices); without it moves go through update_vertices and removals always pass their vertex ranges."""

    def __init__(self, device, scene_name, seed, key12=0, geometry_ops=False, n_ops=0, ops=None, object_copy=True, ledger=None, checks=True):
        assert not (geometry_ops and device < 0)
        self.cfg = dict(device=device, scene_name=scene_name, seed=seed, key12=key12, geometry_ops=geometry_ops, n_ops=n_ops, ops=ops, object_copy=object_copy)
        self.device, self.name, self.seed, self.key12, self.geometry_ops = device, scene_name, seed, key12, geometry_ops
        self.object_copy = bool(object_copy and device >= 0)
        self.script, self.n_ops = ops, (len(ops) if ops is not None else n_ops)
        self.ledger, self.checks = ledger if ledger is not None else Ledger(), checks
        self.rng = np.random.default_rng([BASE, seed])
        mk_scene, mk_cam = SCENES[scene_name]
        self.sc, self.cam = mk_scene(), mk_cam(W, H)
        self.light = add_emitter_material(self.sc)
        self.mgr = self.sc.manager()
        self.mgr.perform_all_scene_updates(self.sc)
        self.bytes_at_start = capi.live_device_bytes()
        self.ctx = self._context()
        if self.object_copy:
            self.ctx.set_object_vertices(self.sc)
        self.motion = bool(device >= 0 and seed % 2)           # odd seeds keep the temporal history through geometry edits
        if self.motion:
            self.ctx.denoise_temporal_set_motion(True)
        self.mode = 0
        self.has_frame = self.has_history = False
        # every node holds the bytes the refit pass writes: a full refit has run since the last upload or rebuild (the device edits write
        # the nodes they touch with that pass)
        self.refit_bytes = False
        self.orc = None
        self.log, self.done = [], []
        self.step = 0
        self.prev_follower = None
        self.nodes_at_upload = len(self.ctx.export_bvh()["nodes"])
        self.last_regraft = None                               # (step, meshes, export after, reports)
        d = self.cam.ray_directions().reshape(-1, 3)
        self.cam_dirs = np.ascontiguousarray(d, dtype=np.float32)

    # ---- contexts
    def _context(self):
        ctx = capi.Context(self.device)
        if self.device >= 0:
            ctx.set_tuning(12, self.key12)
            ctx.resize(W, H)
        ctx.upload_scene(self.sc)
        if self.device >= 0:
            ctx.set_camera(self.cam)
        return ctx

    def close(self):
        if self.orc is not None:
            self.orc.close()
            self.orc = None
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    # ---- the generator: rng and the scene's counts only
    def _pick_meshes(self, most):
        n = len(self.sc.meshes)
        k = min(int(self.rng.integers(1, most + 1)), n)
        return [int(x) for x in self.rng.choice(n, k, replace=False)]

    def _draw(self):
        rng, sc = self.rng, self.sc
        weights = WEIGHTS_DEVICE if self.geometry_ops else WEIGHTS_HOST
        kinds = list(weights)
        kind = str(rng.choice(kinds, p=np.array([weights[k] for k in kinds], dtype=np.float64) / sum(weights.values())))
        if len(sc.meshes) == 0:
            kind = "append"                                    # nothing to edit: never a no-op
        if kind == "append":
            return dict(op="append", n=int(rng.choice(SIZES)), emissive=bool(rng.integers(0, 3) == 0), plain=int(rng.integers(0, 3)),
                        shift=tuple(float(x) for x in rng.uniform(-0.6, 0.6, 3)))
        if kind == "remove":
            return dict(op="remove", meshes=self._pick_meshes(3), ranges=bool(rng.integers(0, 2)))
        if kind == "regraft":
            return dict(op="regraft", meshes=self._pick_meshes(3))
        if kind == "move":
            ms = self._pick_meshes(2)
            reach = 0.6 * PLACE[self.name]["size"]
            return dict(op="move", meshes=ms, delta=[tuple(float(x) for x in rng.uniform(-reach, reach, 3)) for _ in ms],
                        yaw=[float(rng.uniform(-40, 40)) for _ in ms], call=MOVE_CALLS[int(rng.integers(0, 4))], again=bool(rng.integers(0, 2)))
        if kind == "material":
            if rng.integers(0, 2):
                return dict(op="material", mesh=int(rng.integers(0, len(sc.meshes))), material=int(rng.integers(0, len(sc.materials))))
            return dict(op="material", toggle=int(rng.integers(0, len(sc.materials))))
        if kind == "frame":
            return dict(op="frame", tech=TECHS[int(rng.integers(0, len(TECHS)))], rand_seed=int(rng.integers(1, 1 << 30)))
        if kind == "denoise":
            return dict(op="denoise", temporal=bool(rng.integers(0, 3) == 0))
        return dict(op=kind)

    # ---- one op
    def run(self):
        """Every op of the sequence; an assertion failure is raised again with the ops made so far."""
        try:
            while self.step < self.n_ops:
                op = self.script[self.step] if self.script is not None else self._draw()
                self.log.append(" ".join(f"{k}={v}" for k, v in op.items()))
                self._apply(dict(op))
                self.done.append(op)
                self.step += 1
        except (AssertionError, capi.FyprtError) as e:
            raise AssertionError(f"{self.name} seed {self.seed} key 12 = {self.key12}, step {self.step} after {self.log}: {type(e).__name__}: {e}") from e
        return self

    def _follow(self, what):
        if self.prev_follower in TOPOLOGY:
            self.ledger.pairs.add((self.prev_follower, what))
        self.prev_follower = what

    def _apply(self, op):
        kind = op.pop("op")
        if self.checks:
            self.ledger.ops[kind] += 1
        getattr(self, "_op_" + kind)(**op)

    def _export(self):
        return self.ctx.export_bvh() if self.checks else None

    def _fresh_tree_equal(self, after):
        fresh = self._context()
        try:
            e = fresh.export_bvh()
            assert rc.same_export(after, e) if self.key12 == 0 else rc.canonical(after) == rc.canonical(e), "a rebuilt tree is not the upload's"
        finally:
            fresh.close()

    def _op_expect(self, what):
        """(scripted sequences) the shape the script is there to reach"""
        e = self.ctx.export_bvh()
        if what == "empty":
            assert (len(e["nodes"]), len(e["tris"]), e["root"], e["max_stack"]) == (0, 0, 0, 0)
        elif what == "leaf root":
            assert e["root"] < 0 and len(e["nodes"]) == 0 and len(e["tris"]) >= 1
        elif what == "first":
            assert self.last_reports[-1].kind == pr.FIRST
        else:
            assert what == "doubled" and len(e["nodes"]) >= 2 * self.nodes_at_upload

    def _op_append_until_rebuilt(self, shift):
        """(scripted) one-triangle appends at the root until one answers kind 4: about three appends a level, 31 levels"""
        assert self.mode == 0
        checks, self.checks = self.checks, False
        try:
            for k in range(150):
                self._op_append(1, False, 0, shift)
                if self.ctx.last_append_placement().kind == pr.REBUILT:
                    break
        finally:
            self.checks = checks
        after = self.ctx.export_bvh()
        assert self.ctx.last_append_placement().kind == pr.REBUILT, "150 appends at the root and no rebuild"
        self.refit_bytes = False
        if self.checks:
            self.ledger.kinds.add(pr.REBUILT)
            self._fresh_tree_equal(after)
            self._after_edit(after)

    def _op_append(self, n, emissive, plain, shift, fits=False):
        sc, ctx = self.sc, self.ctx
        before = self._export()
        live = capi.live_device_bytes()
        m = append_patch(sc, self.cam, self.name, n, self.light if emissive else plain % len(sc.materials), shift=shift)
        ctx.append_meshes(sc, m)
        assert not fits or capi.live_device_bytes() <= live, "an append of a removed size grew the device memory"
        self.has_frame = self.has_history = False
        self._follow(f"append m{self.mode}")
        if not self.checks:
            return
        after = ctx.export_bvh()
        pl = ctx.last_append_placement()
        self.ledger.kinds.add(int(pl.kind))
        assert pl.mode == self.mode and pl.levels_before == before["max_stack"]
        if pl.mode == 1 and pl.kind != pr.REBUILT:             # the report against the placement rule in numpy, on the scene's own vertices
            t0 = len(sc.triangles) - n
            want = pr.place(before, sc.world_vertices["position"], sc.triangles, (t0, t0 + n), pr.sub_levels(before, after, n))
            assert pr.report_tuple(pl) == want, ("the placement rule", pr.report_tuple(pl), want)
        if pl.kind in (pr.SLOT, pr.PAIR) and pl.mode == 1:
            pr.check_placed_graft(before, after, n, pl)
        elif pl.kind != pr.REBUILT:
            check_graft(before, after, n)
        else:
            self._fresh_tree_equal(after)
            self.refit_bytes = False
        assert pl.levels_after == after["max_stack"]
        if self.nodes_at_upload is not None and len(after["nodes"]) > self.nodes_at_upload and pl.kind != pr.REBUILT:
            # the upload allocated the node arrays to size: a tree with more nodes lives in arrays that grew (in this append or a regraft)
            self.ledger.grew = self.ledger.grew or capi.live_device_bytes() > live
        self._after_edit(after)

    def _op_remove(self, meshes, ranges):
        sc, ctx = self.sc, self.ctx
        before = self._export()
        live = capi.live_device_bytes()
        dead = removed_triangles(sc, meshes)
        sc.init_scene_emissive_triangles()
        ctx.remove_meshes(sc.remove_meshes_from_scene(meshes), with_vertex_ranges=bool(ranges) or not self.object_copy)
        self.has_frame = self.has_history = False
        self._follow("remove")
        if not self.checks:
            return
        after = ctx.export_bvh()
        self.ledger.branches |= check_prune(before, after, dead)
        assert capi.live_device_bytes() <= live, "a removal grew the device memory"
        self._after_edit(after)

    def _op_regraft(self, meshes):
        sc, ctx = self.sc, self.ctx
        before = self._export()
        if self.checks:
            lights = (ctx.export_lighttrees(len(sc.meshes)), ctx.export_emissive())
            readouts = (_state(ctx.last_append_placement), _state(ctx.last_edit_stats))
            denoised = ctx.denoise() if self.has_frame else None
        reports = self.last_reports = ctx.regraft_meshes(meshes)
        self._follow("regraft")
        if any(r.kind == pr.REBUILT for r in reports):
            self.refit_bytes = False
        if not self.checks:
            return
        after = ctx.export_bvh()
        listed = np.zeros(len(sc.triangles), dtype=bool)
        listed[mesh_triangles(sc, meshes)] = True
        tb, ta = before["tris"], after["tris"]
        kept = tb[~listed[tb["tri"]]] if len(tb) else tb
        assert len(ta) == len(tb) and ta[:len(kept)].tobytes() == kept.tobytes(), "leaf records outside the listed meshes moved"
        at = len(kept)
        for m in meshes:
            first, count, _ = sc.meshes[m]
            assert sorted(ta["tri"][at:at + count].tolist()) == list(range(first, first + count)), f"records of mesh {m}"
            at += count
        assert len(reports) == len(meshes) and all(r.mode == self.mode for r in reports)
        with_triangles = [r for r, m in zip(reports, meshes) if sc.meshes[m][1]]
        if with_triangles:
            assert with_triangles[-1].levels_after == after["max_stack"]
            self.ledger.kinds |= {int(r.kind) for r in with_triangles}
            if with_triangles[-1].kind == pr.REBUILT:
                self._fresh_tree_equal(after)
        now = (ctx.export_lighttrees(len(sc.meshes)), ctx.export_emissive())
        for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root"):
            assert lights[0][k].tobytes() == now[0][k].tobytes(), k
        assert lights[0]["tlas_root"] == now[0]["tlas_root"] and np.array_equal(lights[1], now[1])
        assert readouts == (_state(ctx.last_append_placement), _state(ctx.last_edit_stats)), "a regraft moved a readout"
        if denoised is not None:
            again = ctx.denoise()
            assert np.array_equal(denoised[0], again[0]) and bits_equal(denoised[1], again[1]).all(), "the denoised frame changed over a regraft"
        self.last_regraft = (self.step, list(meshes), after, reports)
        self._after_edit(after)

    def _op_move(self, meshes, delta, yaw, call, again):
        sc, ctx = self.sc, self.ctx
        if not self.object_copy:
            call = "update_vertices"
        before = self._export()
        for m, d, y in zip(meshes, delta, yaw):
            p = sc.mesh_transforms[m]["pos"]
            self.mgr.set_mesh_transform(sc, m, pos=tuple(float(p[i]) + d[i] for i in range(3)), rotation=(0.0, y, 0.0))
        self.mgr.perform_all_scene_updates(sc)
        partial = call in (MOVE_CALLS[0], MOVE_CALLS[2])
        if call == MOVE_CALLS[0]:
            ctx.update_mesh_vertices(sc, meshes)
        elif call == MOVE_CALLS[3]:
            ctx.update_vertices(sc)
        else:
            ctx.set_tuning(22, int(partial))
            ctx.update_transforms(sc, meshes)
            ctx.set_tuning(22, 0)
        self.has_frame = False
        self.has_history = self.has_history and self.motion
        self._follow("partial move" if partial else "full move")
        had_refit_bytes = self.refit_bytes
        self.refit_bytes = self.refit_bytes or not partial
        after = None
        if self.checks:
            st = ctx.last_edit_stats()
            self.ledger.partial.add(int(st.partial))
            assert st.partial == int(partial)
            after = ctx.export_bvh()
            if partial:
                tris = mesh_triangles(sc, meshes)
                assert st.triangles_refreshed == len(tris)
                clean = np.ones(len(before["nodes"]), dtype=bool)
                clean[sorted(expected_dirty_nodes(before, tris))] = False
                assert after["nodes"][clean].tobytes() == before["nodes"][clean].tobytes(), "a partial refit wrote a node nothing moved under"
            else:
                assert st.triangles_refreshed == len(sc.triangles)
            assert after["root"] == before["root"] and np.array_equal(after["tris"]["tri"], before["tris"]["tri"])
        if again:
            ctx.update_vertices(sc)                            # the same vertices: a full refit of what the edit left
            self.refit_bytes = True
            if self.checks:
                full = ctx.export_bvh()
                if had_refit_bytes or not partial:
                    assert rc.same_export(after, full), "a full refit of unmoved vertices changed the tree the edit left"
                after = full
        if self.checks:
            self._after_edit(after)

    def _op_material(self, mesh=None, material=None, toggle=None):
        sc, ctx = self.sc, self.ctx
        before = self._export()
        listed = []
        if toggle is None:
            self.mgr.set_mesh_material(sc, mesh, material)
            listed = [mesh]
        else:
            m = sc.materials[toggle]
            emits = float(m.emission_power) > 0 and any(float(c) > 0 for c in m.emission_color)
            sc.materials[toggle] = replace(m, emission_power=0.0) if emits else replace(m, emission_color=(1.0, 0.8, 0.5), emission_power=3.0)
            self.mgr.material_edited(toggle)
        self.mgr.perform_all_scene_updates(sc)
        ctx.update_materials(sc, listed)
        self.has_frame = self.has_history = False
        if self.checks:
            after = ctx.export_bvh()
            assert rc.same_export(before, after), "a material edit touched the tree"
            self._after_edit(after)

    def _op_texture(self):
        sc, ctx = self.sc, self.ctx
        before = self._export()
        slot = len(sc.textures)
        sc.textures.append((np.arange(35, dtype=np.uint32).reshape(5, 7) * np.uint32(0x01020304 + self.step)) | np.uint32(0xFF000000))
        ctx.append_textures(sc.textures[-1:])
        if any(m.is_use_albedo_map and m.albedo_map_index == slot for m in sc.materials):
            self.has_frame = self.has_history = False
        if self.checks:
            assert rc.same_export(before, ctx.export_bvh()), "a texture import touched the tree"

    def _op_mode(self):
        self.mode ^= 1
        self.ctx.set_append_placement(self.mode)

    def _op_cost(self):
        got = rc.cost_tuple(self.ctx.tree_cost())
        if self.checks:
            assert rc.cost_tuple(self.ctx.tree_cost()) == got, "two cost readouts of one tree differ"
            rc.assert_cost_close(got, rc.tree_cost_ref(self.ctx.export_bvh(), self.sc))

    def _op_frame(self, tech, rand_seed):
        from oraclelib import Oracle
        sc, ctx = self.sc, self.ctx
        if len(sc.init_scene_emissive_triangles()) == 0:
            tech = capi.BRDF_SAMPLING                          # no emitter: the light-based techniques answer FYPRT_ENOLIGHT
        st = capi.Settings(technique=tech, sample_count=1, light_bounces=2, sky_color=(0.1, 0.2, 0.3), light_candidate_count=4, use_temporal_reuse=1,
                           use_spatial_reuse=1, temporal_history_limit=3, spatial_neighbor_num=4, spatial_neighbor_radius=12, rand_seed=rand_seed)
        ctx.render(st)
        self.has_frame = True
        if not self.checks:
            return
        old, self.orc = self.orc, Oracle(sc, W, H)
        self.orc.set_camera(self.cam)
        if old is not None:
            self.orc.adopt_frame(old)
            old.close()
        self.orc.use_product_bvh(ctx.export_bvh())
        self.orc.render(st)
        img, acc = ctx.readback()
        ok = bits_equal(acc, self.orc.accum()).all(axis=-1)
        assert ok.all(), f"{(~ok).sum()} accumulation pixels differ from the oracle's"
        assert np.array_equal(img, self.orc.image()), "image"
        if tech in (capi.RESTIR_DI, capi.RESTIR_GI):          # (the per-pixel techniques own no buffer besides accumulation and image)
            for b in (capi.BUF_PAYLOAD, capi.BUF_DEPTH, capi.BUF_DI_PREV if tech == capi.RESTIR_DI else capi.BUF_GI_PREV):
                g, o = ctx.read_buffer(b), self.orc.read_buffer(b)
                e = struct_equal(g, o) if g.dtype.names else bits_equal(g, o)
                assert e.all(), f"buffer {b}: {(~e).sum()} records differ from the oracle's"

    def _refused(self, call):
        try:
            call()
        except capi.FyprtError as e:
            assert _error_code(e) == ESTATE, e
            return
        raise AssertionError(f"{call.__name__} succeeded where the header refuses it (FYPRT_ESTATE)")

    def _op_denoise(self, temporal):
        ctx = self.ctx
        call = ctx.denoise_temporal if temporal else ctx.denoise
        if self.has_frame:
            call()
            self.has_history = self.has_history or temporal
        else:
            self._refused(call)
        if self.has_history:
            ctx.read_buffer(capi.BUF_TEMPORAL)
        else:
            self._refused(lambda: ctx.read_buffer(capi.BUF_TEMPORAL))

    # ---- after every op that changed scene or tree
    def _rays(self):
        n = 128
        o, d = bruteforce.random_rays(self.sc, n, [BASE, self.seed, self.step])
        pick = np.random.default_rng([BASE, self.seed, self.step, 1]).choice(len(self.cam_dirs), n, replace=False)
        eye = np.tile(np.asarray(self.cam.position, dtype=np.float32), (n, 1))
        return np.concatenate([o, eye]), np.concatenate([d, self.cam_dirs[pick]])

    def check_rays(self, export=None):
        """256 rays against the brute force over the scene's own triangles: the device's queries, or the oracle's walk of the export."""
        sc, ctx = self.sc, self.ctx
        if len(sc.triangles) == 0:
            if self.device >= 0:
                eye = np.tile(np.asarray(self.cam.position, dtype=np.float32), (64, 1))
                assert (ctx.trace_rays(eye, self.cam_dirs[:64])["objectIndex"] < 0).all()
            return
        o, d = self._rays()
        truth = _scene_bvh(sc)
        best, _, ties = bruteforce.closest(truth, o, d)
        if self.device >= 0:
            got = ctx.trace_rays(o, d)
            lo = np.full(len(o), 0.05, np.float32)
            assert np.array_equal(ctx.trace_rays(o, d, lo, 3.0, occluded=True), bruteforce.occluded(truth, o, d, lo, 3.0)), "occlusion queries"
        else:
            from oraclelib import Oracle
            walk = Oracle(sc, 8, 8)
            walk.use_product_bvh(export if export is not None else ctx.export_bvh())
            got = np.zeros(len(o), dtype=capi.PAYLOAD_DTYPE)
            for i in range(len(o)):
                got[i] = walk.trace(o[i], d[i])[0]
            walk.close()
        bad = bruteforce.check_closest(got, best, ties)
        assert bad == [], f"{len(bad)} rays differ from the brute force, the first: origin {o[bad[0]].tolist()} direction {d[bad[0]].tolist()}"

    def _after_edit(self, after):
        sc = self.sc
        if len(sc.triangles):
            check_bvh_invariants(after, sc, require_wide=False)
            if after["root"] < 0:
                self.ledger.leaf_root = True
        else:
            assert (len(after["nodes"]), len(after["tris"]), after["root"], after["max_stack"]) == (0, 0, 0, 0), "an emptied scene exports an empty tree"
            self.ledger.emptied = True
        fresh = self._context()
        try:
            same_exports(self.ctx, fresh, len(sc.meshes))
        finally:
            fresh.close()
        self.check_rays(after)

    # ---- the end of a sequence
    def finish(self):
        """Closes the context; then (key 12 = 0) the replay and the twin of the last regraft."""
        final = self.ctx.export_bvh()
        last = self.last_regraft
        self.close()
        assert capi.live_device_bytes() == self.bytes_at_start, "device memory after close"
        if self.key12 != 0:
            return
        again = play(self.cfg, self.n_ops)
        try:
            assert rc.same_export(final, again.ctx.export_bvh()), f"the same ops on a second context left another tree: {self.log}"
        finally:
            again.close()
        if last is None:
            return
        step, meshes, export, reports = last
        start = play(self.cfg, step)
        try:
            twin_export, twin_reports, new_index, _, _ = rc.twin_regraft(start.ctx, start.sc, meshes)
            rc.assert_equals_twin(export, reports, twin_export, twin_reports, new_index, exact=True)
        except AssertionError as e:
            raise AssertionError(f"the twin of the regraft at step {step} of {self.log}: {e}") from e
        finally:
            start.close()


def play(cfg, upto, checks=False):
    """The first `upto` ops of the sequence `cfg` describes, on a new context; returns the open mirror."""
    m = EditMirror(**cfg, checks=checks)
    m.n_ops = upto
    try:
        return m.run()
    except BaseException:
        m.close()
        raise


def run_sequence(ledger, device, scene_name, seed, key12=0, geometry_ops=False, n_ops=0, ops=None, object_copy=True):
    """One sequence with every check, its end-of-sequence checks included."""
    m = EditMirror(device, scene_name, seed, key12, geometry_ops, n_ops=n_ops, ops=ops, object_copy=object_copy, ledger=ledger)
    try:
        m.run()
        m.finish()
    finally:
        m.close()
    return m


def seeds(default_count):
    """Seeds 1 .. default_count; FYPRT_EDITSEQ_FIRST / FYPRT_EDITSEQ_LAST select another range (soak runs)."""
    import os
    if "FYPRT_EDITSEQ_FIRST" in os.environ:
        first = int(os.environ["FYPRT_EDITSEQ_FIRST"])
        return list(range(first, int(os.environ.get("FYPRT_EDITSEQ_LAST", first)) + 1))
    return list(range(1, default_count + 1))


# ---- scripted edge sequences (cornell: meshes 0-7; 5 the tall box, 6 the short box, 2 the back wall).  `device`: with the geometry
# ops and frames a host-only context refuses.
def _append(n, shift=(0.0, 0.0, 0.0), **kw):
    return dict(op="append", n=n, emissive=False, plain=0, shift=shift, **kw)


def _move(meshes, call, again=False, delta=(0.1, 0.05, -0.1), yaw=15.0):
    return dict(op="move", meshes=list(meshes), delta=[delta] * len(meshes), yaw=[yaw] * len(meshes), call=call, again=again)


def _frame(tech=capi.RESTIR_DI):
    return dict(op="frame", tech=tech, rand_seed=7)


def shrink_and_regrow(device, n_meshes=8):
    partial = [_move([0], MOVE_CALLS[0])] if device else []
    return ([dict(op="remove", meshes=list(range(n_meshes)), ranges=True), dict(op="expect", what="empty"),
             _append(1), dict(op="expect", what="leaf root"), dict(op="regraft", meshes=[0]), dict(op="expect", what="first")] + partial +
            [_append(4, (0.3, 0.1, 0.0)), _append(5, (-0.3, -0.1, 0.1)), dict(op="remove", meshes=[0], ranges=True),
             dict(op="regraft", meshes=[0, 1])] + ([_frame(capi.BRDF_SAMPLING)] if device else []))


def grow_past_capacity(device, n_meshes=8):
    partial = [_move([n_meshes], MOVE_CALLS[2])] if device else []
    return ([dict(op="mode")] + [_append(300, (0.25 * k - 0.4, 0.1 * k - 0.1, 0.05 * k)) for k in range(4)] + [dict(op="expect", what="doubled")] + partial +
            [dict(op="remove", meshes=[n_meshes + 1, n_meshes + 2], ranges=False), _append(300, (0.1, -0.2, 0.0), fits=True)] + ([_frame()] if device else []))


def stale_host_vertices():
    """(device) A = 5, B = 6, C = 2: after the removal A = 4, B = 5.  The regraft runs in mode 1 as well: the search reads the box of
    the mesh where it lies now from the host's vertices, so its report (held against the twin's) shows a copy left behind."""
    return [_move([5, 6], MOVE_CALLS[1], delta=(0.3, 0.0, -0.25), yaw=60.0), dict(op="remove", meshes=[2], ranges=False), dict(op="mode"),
            dict(op="regraft", meshes=[4]), _append(5, (-0.35, -0.45, 0.3)), _move([1], MOVE_CALLS[3], delta=(0.0, 0.02, 0.0), yaw=0.0), _frame()]


def links(device):
    """After each topology edit, and after the rebuild an append falls back to, a partial refit must find links of the tree as it is
    now: a partial move, then a full refit of the same vertices with equal bytes (on a tree a full refit has run on)."""
    full = [_move([3], MOVE_CALLS[3], delta=(0.0, 0.0, 0.01), yaw=0.0)] if device else []
    probe = (lambda m: [_move([m], MOVE_CALLS[0], again=True), _move([m], MOVE_CALLS[2], again=True, delta=(-0.05, 0.0, 0.05))]) if device else (lambda m: [])
    return (full + [_append(65, (0.2, 0.2, 0.0))] + probe(8) + [dict(op="remove", meshes=[1], ranges=True)] + probe(7) +
            [dict(op="regraft", meshes=[3, 0])] + probe(3) + [dict(op="append_until_rebuilt", shift=(0.0, -0.3, 0.2))] + full + probe(5))


def grafts_spliced_away(n_meshes=8):
    """Four grafts at the root (a new root that takes two more children, then another new root) removed in one call: a chain of splices
    up to a replaced root, which leaves the uploaded tree's shape; then the placement mode switched back between two appends."""
    shifts = [(0.2 * k - 0.4, 0.1, 0.0) for k in range(4)]
    return ([_append(n, s) for n, s in zip((300, 1, 4, 5), shifts)] + [dict(op="remove", meshes=list(range(n_meshes, n_meshes + 4)), ranges=True),
            dict(op="mode"), _append(5, (0.3, -0.2, 0.1)), dict(op="mode"), _append(4, (-0.3, 0.3, 0.0)), dict(op="cost")])


def removal_after_a_lightless_append(device):
    """Found by the random sequences: an append without an emitter left the light tables at the old scene's size, and the removal of
    fewer triangles than it had brought then sized them by the scene and grew the device memory, against the removal's promise."""
    return [_append(5, (-0.4, -0.27, 0.3)), dict(op="remove", meshes=[2], ranges=False)] + ([_frame(capi.NEE)] if device else [])
