"""The tensor contract between mesh preprocessing and the network, mirroring the reference's
``dataClasses.py`` (PreprocessedData / TrainingSet / InferenceMesh, dataClasses.py:6-27,480-531).

Same attribute names and per-mesh list layout:
    in_list[i]      float64 [1, N0, 6]    unit normal | barycentre / bbox diagonal, fake rows all-zero
    adj_list[i][l]  int64   [1, N_l, 23]  one-indexed K-lists of the 3 graph levels (binary-tree order)
    gt_list[i]      float64 [1, N0, 3]    ground-truth normals (training sets)
    num_faces[i], patch_indices[i], permutations[i] (= inv_perm(newToOld))
    edge_map int32 [1, E, 4], v_e_map int32 [1, V, MAX_EDGES]  (getEdgeMap, for the vertex update)

Differences, by design: the adjacency / coarsening loops run natively (libfgc host routines) and a mesh is
kept whole by default (maxSize = 10^9): the reference cuts meshes above MAX_PATCH_SIZE = 20 000 faces into BFS
patches only because one TF graph could not hold more (settings.py:20-22); a 1M-facet mesh fits one MI355X many times
over.  Constructed with maxSize = MAX_PATCH_SIZE the reference's patch mode is reproduced (same patches for the same
numpy seed; receptive fields truncated at patch borders, overlaps summed at inference).
"""
import numpy as np

from . import utils
from .settings import K_faces, COARSENING_STEPS, COARSENING_LVLS, MIN_PATCH_SIZE, MAX_EDGES


class PreprocessedData(object):
    def __init__(self, maxSize=10 ** 9, coarseningStepNum=COARSENING_STEPS, coarseningLvlNum=COARSENING_LVLS):
        self.in_list = []
        self.gt_list = []
        self.adj_list = []
        self.mesh_count = 0
        self.num_faces = []
        self.patch_indices = []
        self.permutations = []
        self.parents_list = []          # recorded cluster assignments (lets a run be replayed bit-exactly)
        self.maxSize = maxSize
        self.patchSize = maxSize
        self.coarseningStepNum = coarseningStepNum
        self.coarseningLvlNum = coarseningLvlNum
        self.minPatchSize = MIN_PATCH_SIZE
        self.seed = 0
        # multi-scale vertex pipeline (addMeshWithVertices, dataClasses.py:236-456)
        self.v_list = []
        self.faces_list = []
        self.v_faces_list = []
        self.vOldInd_list = []
        self.fOldInd_list = []

    def addMesh_TimeEfficient(self, V0, faces0, GTV=None, seed=None, parents=None):
        """dataClasses.py:34-233: whole mesh (:172-233) or, above maxSize faces, breadth-first patches (:76-171)."""
        V0 = np.asarray(V0, dtype=np.float32)
        faces0 = np.asarray(faces0)
        facesNum = faces0.shape[0]
        # dataClasses.py:40-42: edge tables for the vertex update that follows inference
        try:
            self.edge_map, self.v_e_map = utils.getEdgeMap(faces0, maxEdges=MAX_EDGES)
            self.edge_map = np.expand_dims(self.edge_map, axis=0)
            self.v_e_map = np.expand_dims(self.v_e_map, axis=0)
        except RuntimeError:        # a vertex with more than MAX_EDGES edges: the reference dies here with an
            self.edge_map = self.v_e_map = None   # IndexError; normals can still be inferred, only the vertex update cannot
        f_normals0, f_pos0 = utils.face_features(V0, faces0)
        f_adj0 = utils.getFacesLargeAdj(faces0, K_faces)
        f_normals_pos = np.concatenate((f_normals0, f_pos0), axis=1)        # float64 [F,6] (dataClasses.py:64)
        GTf_normals0 = utils.computeFacesNormals(GTV, faces0) if GTV is not None else None
        if facesNum > self.maxSize:
            # dataClasses.py:76-171: breadth-first patches of patchSize faces (already covered faces join as context),
            # seeds drawn with numpy's global RNG among the uncovered faces unless the previous patch proposed one
            print("Dividing mesh into patches: %i faces (%i max allowed)" % (facesNum, self.maxSize))
            faceCheck = np.zeros(facesNum)
            faceRange = np.arange(facesNum)
            nextSeed = -1
            while np.any(faceCheck == 0):
                toBeProcessed = faceRange[faceCheck == 0]
                faceSeed = toBeProcessed[np.random.randint(toBeProcessed.shape[0])] if nextSeed == -1 else nextSeed
                patchAdj, fOldInd, nextSeed = utils.getGraphPatch_wMask(f_adj0, self.patchSize, faceSeed, faceCheck,
                                                                        self.minPatchSize)
                faceCheck[fOldInd] = 1
                if fOldInd.shape[0] < 100:      # small disjoint components are dropped (dataClasses.py:103-104)
                    continue
                self._add_graph(patchAdj, f_normals_pos[fOldInd],
                                GTf_normals0[fOldInd] if GTf_normals0 is not None else None, fOldInd, seed, parents)
        else:
            self._add_graph(f_adj0, f_normals_pos, GTf_normals0, [], seed, parents)

    def addMeshWithVertices(self, V0, faces0, GTV=None, seed=None, parents=None):
        """dataClasses.py:236-456, whole-mesh branch (:374-440): what the multi-scale network + update_position_MS
        consume.  On top of addMesh_TimeEfficient: the faces padded with -1 rows for the fake nodes and re-ordered like
        the nodes (faces_list), the node ids of the faces around every vertex (v_faces_list, 25 slots) and the vertices
        divided by the bounding-box diagonal (v_list).  Returns (vNum, facesNum)."""
        V0 = np.asarray(V0, dtype=np.float32)
        faces0 = np.asarray(faces0)
        if faces0.shape[0] > self.maxSize:
            return self._add_mesh_patches_with_vertices(V0, faces0, GTV, seed)
        first = len(self.in_list)
        self.addMesh_TimeEfficient(V0, faces0, GTV=GTV, seed=seed, parents=parents)
        oldToNew = self.permutations[first]
        new_N = len(oldToNew)
        newToOld = np.empty(new_N, dtype=np.int64)
        newToOld[oldToNew] = np.arange(new_N)
        faces_p = np.concatenate((faces0.astype(np.int64), -np.ones((new_N - faces0.shape[0], 3), dtype=np.int64)),
                                 axis=0)[newToOld]
        v_faces = utils.getVerticesFaces(faces_p, 25, V0.shape[0])
        if GTV is not None:
            Vn, GTn = utils.normalizePointSets(V0, np.asarray(GTV, dtype=np.float32))
            self.__dict__.setdefault("gtv_list", []).append(GTn[np.newaxis])
        else:
            Vn, _ = utils.normalizePointSets(V0, V0)
        self.v_list.append(Vn[np.newaxis])
        self.faces_list.append(faces_p[np.newaxis])
        self.v_faces_list.append(v_faces[np.newaxis])
        self.fOldInd_list.append([])
        self.vOldInd_list.append([])
        return V0.shape[0], faces0.shape[0]

    def _add_mesh_patches_with_vertices(self, V0, faces0, GTV, seed):
        """dataClasses.py:270-372: meshes above maxSize are cut into breadth-first MESH patches (getMeshPatch) around
        seeds drawn with np.random among the faces no patch has covered yet, until every face is covered; components of
        fewer than 100 faces are dropped, and with a ground-truth point cloud so are patches whose bounding box holds
        fewer GT points than the patch has vertices.  Every patch brings its own vertices (normalised coordinates),
        faces, vertex-face table and graph levels; vOldInd_list / fOldInd_list map them back."""
        f_normals0 = utils.computeFacesNormals(V0, faces0)
        f_adj0 = utils.getFacesLargeAdj(faces0, K_faces)
        f_pos0 = utils.getTrianglesBarycenter(V0, faces0, normalize=True)
        f_normals_pos = np.concatenate((f_normals0, f_pos0), axis=1)
        addGT = GTV is not None
        if addGT:
            GTV = np.asarray(GTV, dtype=np.float32)
            gtf_normals0 = utils.computeFacesNormals(GTV, faces0)
            Vn, GTn = utils.normalizePointSets(V0, GTV)
        else:
            Vn, _ = utils.normalizePointSets(V0, V0)
        facesNum = faces0.shape[0]
        faceCheck = np.zeros(facesNum)
        faceRange = np.arange(facesNum)
        while np.any(faceCheck == 0):
            toBeProcessed = faceRange[faceCheck == 0]
            faceSeed = toBeProcessed[np.random.randint(toBeProcessed.shape[0])]
            pV, pF, pAdj, vOldInd, fOldInd = utils.getMeshPatch(Vn, faces0, f_adj0, self.patchSize, faceSeed)
            faceCheck[fOldInd] += 1
            if fOldInd.shape[0] < 100:          # small disjoint components are not added
                continue
            if addGT:
                patchGTV = utils.takePointSetSlice(GTn, utils.getBoundingBox(pV))
                if patchGTV.shape[0] < pV.shape[0]:     # no ground truth in the window: a fake surface
                    continue
            first = len(self.in_list)
            self._add_graph(pAdj, f_normals_pos[fOldInd], gtf_normals0[fOldInd] if addGT else None, fOldInd, seed, None)
            oldToNew = self.permutations[first]
            new_N = len(oldToNew)
            newToOld = np.empty(new_N, dtype=np.int64)
            newToOld[oldToNew] = np.arange(new_N)
            faces_p = np.concatenate((pF.astype(np.int64), -np.ones((new_N - pF.shape[0], 3), dtype=np.int64)),
                                     axis=0)[newToOld]
            self.v_list.append(pV[np.newaxis])
            self.faces_list.append(faces_p[np.newaxis])
            self.v_faces_list.append(utils.getVerticesFaces(faces_p, 25, pV.shape[0])[np.newaxis])
            self.vOldInd_list.append(vOldInd)
            self.fOldInd_list.append(fOldInd)
            if addGT:
                self.__dict__.setdefault("gtv_list", []).append(patchGTV[np.newaxis])
        return V0.shape[0], facesNum

    def _add_graph(self, f_adj, f_normals_pos, GTf_normals, patch_index, seed, parents):
        """One mesh or one patch: coarsen, pad with fake nodes, reorder, append (dataClasses.py:106-171,172-233)."""
        old_N = f_adj.shape[0]
        f_normals0, f_pos0 = f_normals_pos[:, :3], f_normals_pos[:, 3:]
        GTf_normals0 = GTf_normals
        if self.coarseningLvlNum > 1:
            levels = (self.coarseningLvlNum - 1) * self.coarseningStepNum
            keep = tuple(self.coarseningStepNum * l for l in range(self.coarseningLvlNum))
            cur_seed = self.seed if seed is None else seed
            has_sat = True
            while has_sat:      # dataClasses.py:179-192: re-draw the pairing while a row saturates K
                klists, newToOld, par, has_sat = utils.coarsen_klists(f_adj, f_pos0, f_normals0, levels, K_faces,
                                                                      cur_seed, parents, keep)
                if has_sat and parents is not None:
                    raise RuntimeError("recorded cluster assignments saturate K=%d" % K_faces)
                cur_seed += 1
            self.seed = cur_seed
            fAdjs = [k[np.newaxis].astype(np.int64) for k in klists]
            new_N = len(newToOld)
            pad6 = np.zeros((new_N - old_N, f_normals_pos.shape[1]))
            f_normals_pos = np.concatenate((f_normals_pos, pad6), axis=0)[newToOld]
            if GTf_normals0 is not None:
                GTf_normals0 = np.concatenate((GTf_normals0, np.zeros((new_N - old_N, 3))), axis=0)[newToOld]
            self.parents_list.append(par)
        else:
            fAdjs = [f_adj[np.newaxis].astype(np.int64)]
            newToOld = None
        self.num_faces.append(old_N)
        self.patch_indices.append(patch_index)
        if newToOld is not None:
            self.permutations.append(utils.inv_perm(newToOld))
        self.in_list.append(f_normals_pos[np.newaxis])
        self.adj_list.append(fAdjs)
        if GTf_normals0 is not None:
            self.gt_list.append(np.asarray(GTf_normals0, dtype=np.float64)[np.newaxis])
        self.mesh_count += 1


class TrainingSet(PreprocessedData):
    """dataClasses.py:480-506 (array interface; OBJ parsing is outside the hot path)."""

    def addMeshWithGT(self, V_noisy, faces, V_gt, seed=None, parents=None):
        """dataClasses.py:490-494.  Either the reference's call addMeshWithGT(inputFilePath, filename, gtFilePath,
        gtfilename) (both OBJs are read with utils.load_mesh; the faces of the noisy file are used for both) or arrays
        addMeshWithGT(V_noisy, faces, V_gt)."""
        if isinstance(V_noisy, str):
            in_path, in_name, gt_path, gt_name = V_noisy, faces, V_gt, seed
            V_noisy, _, _, faces, _ = utils.load_mesh(in_path, in_name, 0, False)
            V_gt = utils.load_mesh(gt_path, gt_name, 0, False)[0]
            seed = None
        self.addMesh_TimeEfficient(V_noisy, faces, GTV=V_gt, seed=seed, parents=parents)

    def addCleanMesh(self, V, faces, seed=None, parents=None):
        """Build extension (no counterpart in the reference): a CLEAN mesh for training on noise synthesised per step on the
        GPU (FacetDenoiser.bind_clean).  Arrays addCleanMesh(V, faces) or the file form addCleanMesh(path, filename).
        Everything addMeshWithGT(V, faces, V) does - the mesh's own rows in in_list, its normals in gt_list - plus, per
        mesh, clean_vertices (float32 [1, V, 3]), clean_faces_rows (int32 [1, N0, 3]: the faces padded with -1 rows for
        the fake nodes and reordered like the nodes, as addMeshWithVertices builds faces_list) and clean_edge_len (the
        mean edge length, utils.getAverageEdgeLength: a noise level is a multiple of it).
        The graph levels are built from the CLEAN mesh.  The reference coarsens the noisy one; its edge weights are
        almost always the floor value, so the pairing is decided by the random visiting order
        and the clean mesh's levels are another valid draw of the same procedure.
        A mesh above maxSize faces (patch mode) is refused: patches are not synthesised."""
        if isinstance(V, str):
            V, _, _, faces, _ = utils.load_mesh(V, faces, 0, False)
            seed = parents = None
        V = np.ascontiguousarray(np.asarray(V, dtype=np.float32))
        faces = np.asarray(faces)
        if faces.shape[0] > self.maxSize:
            raise NotImplementedError("addCleanMesh keeps a mesh whole: %d faces > maxSize %d (patch mode)"
                                      % (faces.shape[0], self.maxSize))
        first = len(self.in_list)
        self.addMesh_TimeEfficient(V, faces, GTV=V, seed=seed, parents=parents)
        oldToNew = self.permutations[first]
        new_N = len(oldToNew)
        newToOld = np.empty(new_N, dtype=np.int64)
        newToOld[oldToNew] = np.arange(new_N)
        faces_p = np.concatenate((faces.astype(np.int64), -np.ones((new_N - faces.shape[0], 3), dtype=np.int64)),
                                 axis=0)[newToOld]
        for name, value in (("clean_vertices", V[np.newaxis]), ("clean_faces_rows", faces_p.astype(np.int32)[np.newaxis]),
                            ("clean_edge_len", float(utils.getAverageEdgeLength(V, faces)[0]))):
            self.__dict__.setdefault(name, []).append(value)

    def addCleanMeshWithVertices(self, V, faces, seed=None, parents=None):
        """Build extension: a CLEAN mesh for training the vertex networks (trainAccuracyNet / trainDoubleLossNet with
        noise_levels=...) on noise synthesised per step on the GPU (FacetDenoiser.bind_clean_vertices).  Arrays
        addCleanMeshWithVertices(V, faces) or the file form addCleanMeshWithVertices(path, filename).  Everything
        addMeshWithVerticesAndGT(V, faces, V) does - the clean mesh is its own ground truth in gtv_list and gt_list - plus
        the three per-mesh fields of addCleanMesh: clean_vertices (the RAW vertices, float32 [1, V, 3]), clean_faces_rows
        (int32 [1, N0, 3], the values of faces_list) and clean_edge_len.  Patch mode (more faces than maxSize) is refused."""
        if isinstance(V, str):
            V, _, _, faces, _ = utils.load_mesh(V, faces, 0, False)
            seed = parents = None
        V = np.ascontiguousarray(np.asarray(V, dtype=np.float32))
        faces = np.asarray(faces)
        if faces.shape[0] > self.maxSize:
            raise NotImplementedError("addCleanMeshWithVertices keeps a mesh whole: %d faces > maxSize %d (patch mode)"
                                      % (faces.shape[0], self.maxSize))
        self.addMeshWithVerticesAndGT(V, faces, V, seed=seed, parents=parents)
        for name, value in (("clean_vertices", V[np.newaxis]), ("clean_faces_rows", self.faces_list[-1].astype(np.int32)),
                            ("clean_edge_len", float(utils.getAverageEdgeLength(V, faces)[0]))):
            self.__dict__.setdefault(name, []).append(value)

    def is_clean(self):
        """Every mesh of the set came through addCleanMesh or addCleanMeshWithVertices (what noise_levels=... needs)."""
        n = len(self.in_list)
        return n > 0 and all(len(self.__dict__.get(k, ())) == n for k in ("clean_vertices", "clean_faces_rows",
                                                                            "clean_edge_len"))

    def addMeshWithVerticesAndGT(self, V_noisy, faces, V_gt, gtfilename=None, seed=None, parents=None):
        """dataClasses.py:497-506: addMeshWithVertices with the ground-truth vertices (gtv_list), for trainAccuracyNet.
        Either the reference's call addMeshWithVerticesAndGT(inputFilePath, filename, gtFilePath, gtfilename) (both
        OBJs read with utils.load_mesh; the noisy file's faces are used) or arrays addMeshWithVerticesAndGT(V_noisy,
        faces, V_gt)."""
        if isinstance(V_noisy, str):
            in_path, in_name, gt_path = V_noisy, faces, V_gt
            V_noisy, _, _, faces, _ = utils.load_mesh(in_path, in_name, 0, False)
            V_gt = utils.load_mesh(gt_path, gtfilename, 0, False)[0]
        V_noisy = np.asarray(V_noisy, dtype=np.float32)
        self.fNum, self.vNum = np.asarray(faces).shape[0], V_noisy.shape[0]
        PreprocessedData.addMeshWithVertices(self, V_noisy, faces, GTV=V_gt, seed=seed, parents=parents)
        self.vertices = V_noisy[np.newaxis]
        self.faces = np.asarray(faces)
        self.normals = utils.computeFacesNormals(V_noisy, self.faces)

    def addMeshWithVerticesAndGTMesh(self, V_noisy, faces, V_gt, F_gt, seed=None, parents=None):
        """Build extension: a noisy mesh with a ground-truth MESH of any topology, for trainAccuracyNet - its vertex and face
        counts need not be the noisy mesh's, and nothing pairs its facets with the noisy ones.  Arrays
        addMeshWithVerticesAndGTMesh(V_noisy, faces, V_gt, F_gt) or the file form (inputFilePath, filename, gtFilePath,
        gtfilename), each OBJ read with its OWN faces.  Everything addMeshWithVertices(V_noisy, faces) does, with v_list and
        gtv_list normalised together (utils.normalizePointSets(V_noisy, V_gt)) and the ground-truth faces in gtf_list
        (int32 [1, Fgt, 3], one entry per mesh of the set; [1, 0, 3] for a mesh added without).  NO gt_list entry: there
        are no face normals of another topology, so trainNet and the double loss do not take such a set.  Patch mode (more
        faces than maxSize) is refused."""
        if isinstance(V_noisy, str):
            in_path, in_name, gt_path, gt_name = V_noisy, faces, V_gt, F_gt
            V_noisy, _, _, faces, _ = utils.load_mesh(in_path, in_name, 0, False)
            V_gt, _, _, F_gt, _ = utils.load_mesh(gt_path, gt_name, 0, False)
            seed = parents = None
        V_noisy = np.ascontiguousarray(np.asarray(V_noisy, dtype=np.float32)).reshape(-1, 3)
        V_gt = np.ascontiguousarray(np.asarray(V_gt, dtype=np.float32)).reshape(-1, 3)
        faces, F_gt = np.asarray(faces), np.asarray(F_gt)
        if faces.shape[0] > self.maxSize:
            raise NotImplementedError("addMeshWithVerticesAndGTMesh keeps a mesh whole: %d faces > maxSize %d (patch mode)"
                                      % (faces.shape[0], self.maxSize))
        if F_gt.ndim != 2 or F_gt.shape[1] != 3 or F_gt.shape[0] == 0 or V_gt.shape[0] == 0:
            raise ValueError("the ground-truth mesh needs vertices [Vgt,3] and faces [Fgt,3], got %r and %r"
                             % (V_gt.shape, F_gt.shape))
        if F_gt.min() < 0 or F_gt.max() >= V_gt.shape[0]:
            raise ValueError("the ground-truth faces index %d vertices, ids run from %d to %d"
                             % (V_gt.shape[0], F_gt.min(), F_gt.max()))
        first = len(self.in_list)
        self.fNum, self.vNum = faces.shape[0], V_noisy.shape[0]
        PreprocessedData.addMeshWithVertices(self, V_noisy, faces, seed=seed, parents=parents)
        Vn, GTn = utils.normalizePointSets(V_noisy, V_gt)
        self.v_list[-1] = Vn[np.newaxis]        # (addMeshWithVertices normalised the noisy mesh by its own box)
        gtv, gtf = (self.__dict__.setdefault(k, []) for k in ("gtv_list", "gtf_list"))
        if len(gtv) != first:
            raise ValueError("the set holds %d meshes and %d ground-truth vertex sets: a mesh was added without one"
                             % (first, len(gtv)))
        gtf.extend(np.zeros((1, 0, 3), dtype=np.int32) for _ in range(first - len(gtf)))
        gtv.append(GTn[np.newaxis])
        gtf.append(np.ascontiguousarray(F_gt.astype(np.int32))[np.newaxis])
        self.vertices = V_noisy[np.newaxis]
        self.faces = faces
        self.normals = utils.computeFacesNormals(V_noisy, faces)


class InferenceMesh(PreprocessedData):
    """dataClasses.py:510-531."""

    def addMesh(self, V, faces, seed=None, parents=None):
        """dataClasses.py:513-519.  Either the reference's call addMesh(inputFilePath, filename) (an OBJ is read with
        utils.load_mesh) or arrays addMesh(V, faces)."""
        if isinstance(V, str):
            V, _, _, faces, _ = utils.load_mesh(V, faces, 0, False)
        self.vertices = np.asarray(V, dtype=np.float32)[np.newaxis]
        self.faces = np.asarray(faces)
        self.addMesh_TimeEfficient(V, faces, seed=seed, parents=parents)
        self.normals = utils.computeFacesNormals(self.vertices[0], self.faces)

    def addMeshWithVertices(self, V, faces=None, seed=None, parents=None):
        """dataClasses.py:521-531 (file form addMeshWithVertices(inputFilePath, filename), or arrays)."""
        if isinstance(V, str):
            V, _, _, faces, _ = utils.load_mesh(V, faces, 0, False)
        V = np.asarray(V, dtype=np.float32)
        self.fNum, self.vNum = np.asarray(faces).shape[0], V.shape[0]
        PreprocessedData.addMeshWithVertices(self, V, faces, seed=seed, parents=parents)
        self.vertices = V[np.newaxis]
        self.faces = np.asarray(faces)
        self.normals = utils.computeFacesNormals(V, self.faces)
        return self.vNum, self.fNum
