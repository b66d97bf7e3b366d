"""mcrt_group_*: several GPUs of one node behind the C-ABI (the frame loop main.cpp:92-152 sharded by scan-line).
On the one-GPU box a group lists device 0 several times: its ranks then share the GPU, every code path of the real thing runs
(the ranks' host threads, shard ranges, block buffers, peer copies, the interleaving kernel, the double buffering) except the
xGMI hop itself."""
import ctypes as C
import numpy as np
import pytest


def test_shard_rule_and_argument_errors(mcrt):
    """mcrt_group_shard == dist.shard_range (contiguous blocks, the first E % G ranks one more); bad arguments are refused; without
    a GPU the group fails as loudly as a context"""
    from mcray_tracing_amd.dist import shard_range
    for E in (1, 7, 128, 512, 1000):
        for G in (1, 2, 3, 8, 64):
            cover = []
            for r in range(G):
                assert mcrt.shard_range(r, G, E) == shard_range(r, G, E)
                cover += list(range(*mcrt.shard_range(r, G, E)))
            assert cover == list(range(E))
    L = mcrt.load_library()
    b = C.c_uint32(); e = C.c_uint32()
    assert L.mcrt_group_shard(3, 3, 10, C.byref(b), C.byref(e)) == -1
    assert L.mcrt_group_shard(0, 0, 10, C.byref(b), C.byref(e)) == -1
    h = C.c_void_p()
    assert L.mcrt_group_create(None, 2, C.byref(h)) == -1 and h.value is None
    assert L.mcrt_group_size(None) == 0 and L.mcrt_group_root(None) is None
    assert L.mcrt_group_trace_frames(None, 0, 1, None) == -1 and b"null group" in L.mcrt_last_error()
    assert L.mcrt_group_synchronize(None) == -1 and L.mcrt_group_destroy(None) == 0
    if L.mcrt_device_count() == 0:
        with pytest.raises(mcrt.McrtError) as ex:
            mcrt.Group([0, 0])
        assert ex.value.code == -4 and "no CPU fallback" in str(ex.value)


def _setup(obj, mcrt, sd, tr, S, tex, **params):
    obj.set_params(n_elements=tr.n_elements, n_samples=S, frequency=tr.frequency, **params)
    obj.upload_scene(sd)
    obj.upload_texture(tex, 256)
    obj.set_transducer(tr.pos, tr.dir)


@pytest.mark.gpu
@pytest.mark.parametrize("ranks,E", [(2, 16), (3, 16), (1, 8)])
def test_group_equals_single_context(mcrt, sphere, tex256, ranks, E):
    """a group of `ranks` contexts on GPU 0 (even and ragged shards, and the one-rank group) == one context, bit for bit: one frame,
    the frames of a pass, successive passes on alternating buffers (the double buffering), a pass with a probe pose per frame, and
    the whole B-mode frame post-processed on the root context"""
    cfg, sd = sphere
    S = 64
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    one = mcrt.Context(0); _setup(one, mcrt, sd, tr, S, tex256)
    grp = mcrt.Group([0] * ranks); _setup(grp, mcrt, sd, tr, S, tex256)
    assert grp.size == ranks
    R = one.params.n_rows
    psf = mcrt.Psf(freq=tr.frequency)
    F = 3
    ref_dev = one.alloc(F * E * R * 4)
    bufs = [grp.root.alloc(F * E * R * 4) for _ in range(2)]
    img_one, img_grp = one.alloc(F * 400 * 500 * 4), grp.root.alloc(F * 400 * 500 * 4)

    def single(frame, nf):
        one.trace_frames(frame, nf, ref_dev)
        return one.d2h(ref_dev, (nf, E, R))

    # one frame (blocks land in place), then passes of 3 on alternating buffers WITHOUT synchronising in between
    grp.trace_frames(7, 1, bufs[0]); grp.synchronize()
    assert np.array_equal(grp.root.d2h(bufs[0], (1, E, R)).view(np.uint32), single(7, 1).view(np.uint32))
    want = [single(10 + 3 * k, F) for k in range(4)]
    got = []
    for k in range(4):
        grp.trace_frames(10 + 3 * k, F, bufs[k & 1])
        if k >= 1:      # the previous pass's frames, read on the ROOT's stream while this pass is in flight
            got.append(grp.root.d2h(bufs[(k - 1) & 1], (F, E, R)))
    grp.synchronize()
    got.append(grp.root.d2h(bufs[1], (F, E, R)))
    for k in range(4):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.abs(want[0]).sum() > 0 and not np.array_equal(want[0], want[1])
    t_ms, c_ms = grp.last_pass_ms()
    assert (t_ms > 0).all() and (c_ms >= 0).all()

    # the whole B-mode frame: PSF, envelope, scan conversion of the gathered frames on the root context
    for ctx, dev, img in ((one, ref_dev, img_one), (grp.root, bufs[0], img_grp)):
        if ctx is one:
            one.trace_frames(30, F, dev)
        else:
            grp.trace_frames(30, F, dev)
        ctx.convolve_frames(dev, F, E, R, psf.axial_kernel, psf.lateral_kernel)
        ctx.envelope_frames(dev, F, E, R)
        ctx.scan_convert_frames(dev, F, E, R, img)
    grp.synchronize(); one.synchronize()
    a, b = one.d2h(img_one, (F, 400, 500)), grp.root.d2h(img_grp, (F, 400, 500))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.abs(a).sum() > 0

    # a probe pose per frame of the pass
    poses = [mcrt.Transducer(E, position=np.asarray(cfg["transducerPosition"], np.float64) + np.array([0.0, 0.2 * f, 0.0]),
                             angles_deg=np.asarray(cfg["transducerAngles"], np.float64) + np.array([2.0 * f, 0.0, -1.0 * f])) for f in range(F)]
    pos = np.stack([t.pos for t in poses]); dirs = np.stack([t.dir for t in poses])
    one.trace_frames_poses(50, pos, dirs, ref_dev)
    grp.trace_frames_poses(50, pos, dirs, bufs[1]); grp.synchronize()
    assert np.array_equal(one.d2h(ref_dev, (F, E, R)).view(np.uint32), grp.root.d2h(bufs[1], (F, E, R)).view(np.uint32))

    # a rank's error comes back with its rank: a transducer of the wrong size is refused when the pass is traced
    grp.set_transducer(tr.pos[:4], tr.dir[:4])
    with pytest.raises(mcrt.McrtError, match=r"rank 0: transducer has 4 elements"):
        grp.trace_frames(0, 1, bufs[0])
    grp.set_transducer(tr.pos, tr.dir)
    grp.trace_frames(7, 1, bufs[0]); grp.synchronize()
    assert np.array_equal(grp.root.d2h(bufs[0], (1, E, R)).view(np.uint32), single(7, 1).view(np.uint32))
    for d in bufs + [img_grp]:
        grp.root.free(d)
    one.free(ref_dev); one.free(img_one)
    grp.close(); one.close()


@pytest.mark.gpu
def test_group_resources_through_failure_and_regrowth(mcrt, sphere, tex256):
    """a group that fails half-way through its creation (its second rank names a device that does not exist) releases what it had made and
    the next group works; passes of 3, 5 (both staged) and 1 frames (the blocks land in place), then 3 and 5 again -- successive passes alternate
    between the two buffer slots, so it is the LAST pass that grows buffers made for 3 frames to 5; a second group made after the first was
    closed gives the same frames.  All bit for bit one context's."""
    cfg, sd = sphere
    E, S = 16, 32
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    one = mcrt.Context(0); _setup(one, mcrt, sd, tr, S, tex256)
    R = one.params.n_rows
    ref_dev = one.alloc(5 * E * R * 4)
    want = {}
    for F in (3, 5, 1):
        one.trace_frames(20, F, ref_dev)
        want[F] = one.d2h(ref_dev, (F, E, R))
    assert np.abs(want[3]).sum() > 0
    one.free(ref_dev); one.close()

    n = mcrt.load_library().mcrt_device_count()
    with pytest.raises(mcrt.McrtError) as ex:
        mcrt.Group([0, n])
    assert ex.value.code == -1 and "out of range" in str(ex.value)

    def passes(frames):
        grp = mcrt.Group([0, 0]); _setup(grp, mcrt, sd, tr, S, tex256)
        dev = grp.root.alloc(5 * E * R * 4)
        try:
            for F in frames:
                grp.trace_frames(20, F, dev); grp.synchronize()
                assert np.array_equal(grp.root.d2h(dev, (F, E, R)).view(np.uint32), want[F].view(np.uint32)), F
        finally:
            grp.root.free(dev)
            grp.close()

    passes((3, 5, 1, 3, 5))
    passes((3,))


@pytest.mark.gpu
def test_group_moving_geometry_and_device_builder(mcrt, sphere, tex256):
    """mcrt_group_set_bvh_builder / _update_triangles / _refit_triangles reach every rank: frames equal a single context's"""
    cfg, sd = sphere
    E, S, F = 12, 32, 2
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    one = mcrt.Context(0); one.set_bvh_builder("lbvh"); _setup(one, mcrt, sd, tr, S, tex256)
    grp = mcrt.Group([0, 0]); grp.set_bvh_builder("lbvh"); _setup(grp, mcrt, sd, tr, S, tex256)
    R = one.params.n_rows
    a_dev, b_dev = one.alloc(F * E * R * 4), grp.root.alloc(F * E * R * 4)
    moved = sd.tri.reshape(-1, 9) + np.float32(0.05)
    for step, (f1, fg) in enumerate(((None, None), (one.refit_triangles, grp.refit_triangles), (one.update_triangles, grp.update_triangles))):
        if f1:
            f1(moved * np.float32(1.0 + 0.01 * step)); fg(moved * np.float32(1.0 + 0.01 * step))
        one.trace_frames(3, F, a_dev); grp.trace_frames(3, F, b_dev); grp.synchronize()
        assert np.array_equal(one.d2h(a_dev, (F, E, R)).view(np.uint32), grp.root.d2h(b_dev, (F, E, R)).view(np.uint32)), step
    one.free(a_dev); grp.root.free(b_dev)
    grp.close(); one.close()


@pytest.mark.gpu
def test_group_builds_the_host_tree_once(mcrt, sphere, tex256):
    """host SAH builder (the default): mcrt_group_upload_scene / _update_triangles build the tree ONCE on the calling thread and every rank
    installs a copy -- frames equal a single context's that built its own; the device builder needs no host build; scene data must be host
    memory; parameters a context refuses leave the whole group on the old ones"""
    cfg, sd = sphere
    E, S, F = 12, 32, 2
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    one = mcrt.Context(0); _setup(one, mcrt, sd, tr, S, tex256)
    grp = mcrt.Group([0, 0, 0]); _setup(grp, mcrt, sd, tr, S, tex256)
    build_s, upload_s = grp.last_scene_seconds()
    assert build_s > 0 and upload_s > 0
    n1 = one.get_bvh()[0]
    for r in range(3):                                            # every rank holds the SAME tree the single context built for itself
        assert np.array_equal(grp.members[r].get_bvh()[0], n1)
    R = one.params.n_rows
    a_dev, b_dev = one.alloc(F * E * R * 4), grp.root.alloc(F * E * R * 4)
    moved = (sd.tri.reshape(-1, 9) * np.float32(1.02) + np.float32(0.03)).astype(np.float32)
    for step in range(2):
        if step:
            one.update_triangles(moved); grp.update_triangles(moved)
            assert grp.last_scene_seconds()[0] > 0
        one.trace_frames(3, F, a_dev); grp.trace_frames(3, F, b_dev); grp.synchronize()
        assert np.array_equal(one.d2h(a_dev, (F, E, R)).view(np.uint32), grp.root.d2h(b_dev, (F, E, R)).view(np.uint32)), step
    # a device pointer belongs to one GPU: refused by every scene call of the group
    d_tri = grp.root.alloc(moved.nbytes); grp.root.h2d(d_tri, moved)
    L = mcrt.load_library()
    assert L.mcrt_group_update_triangles(grp.h, C.c_void_p(d_tri), moved.shape[0]) == -1 and b"host memory" in L.mcrt_last_error()
    meshes = (mcrt.MeshRec * len(sd.meshes))(*[mcrt.MeshRec(a, b, c, 0) for a, b, c in sd.meshes])
    sp = np.asarray(sd.spacing, np.float32); tm = np.ascontiguousarray(sd.tri_mesh, np.uint32); mats = np.ascontiguousarray(sd.materials, np.float32)
    assert L.mcrt_group_upload_scene(grp.h, C.c_void_p(d_tri), tm.ctypes.data_as(C.c_void_p), moved.shape[0], meshes, len(sd.meshes),
                                     mats.ctypes.data_as(C.c_void_p), mats.shape[0], sd.start_mat, sp.ctypes.data_as(C.c_void_p)) == -1
    assert b"host memory" in L.mcrt_last_error()
    grp.root.free(d_tri)
    # refused parameters: nobody keeps them
    with pytest.raises(mcrt.McrtError):
        grp.set_params(n_rows=0)
    assert grp.root.params.n_rows == R and all(grp.members[r].params.n_rows == R for r in range(3))
    grp.trace_frames(3, F, b_dev); grp.synchronize()
    assert np.array_equal(one.d2h(a_dev, (F, E, R)).view(np.uint32), grp.root.d2h(b_dev, (F, E, R)).view(np.uint32))
    # the device builder: no host build
    grp.set_bvh_builder("lbvh"); grp.upload_scene(sd)
    assert grp.last_scene_seconds()[0] < 1e-3
    one.free(a_dev); grp.root.free(b_dev)
    grp.close(); one.close()


@pytest.mark.gpu
def test_group_on_two_devices(mcrt, sphere, tex256):
    """the xGMI half of mcrt_group -- hipMemcpyPeerAsync into the root's buffer, peer access, the root's stream waiting on events recorded on
    ANOTHER device's stream -- needs two GPUs: runs where the box has them (the one-GPU test box skips; until it has run there, that hop is
    verified by reading only -- README / INTEGRATION say so)"""
    if mcrt.load_library().mcrt_device_count() < 2:
        pytest.skip("one GPU: the peer-copy path between DEVICES cannot run here")
    cfg, sd = sphere
    E, S, F = 13, 64, 3                                            # ragged: 7 + 6 scan-lines
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    one = mcrt.Context(0); _setup(one, mcrt, sd, tr, S, tex256)
    grp = mcrt.Group([0, 1]); _setup(grp, mcrt, sd, tr, S, tex256)
    R = one.params.n_rows
    a_dev = one.alloc(F * E * R * 4); bufs = [grp.root.alloc(F * E * R * 4) for _ in range(2)]
    for k in range(4):                                             # successive passes on alternating buffers, no synchronisation in between
        grp.trace_frames(10 + 3 * k, F, bufs[k & 1])
    grp.synchronize()
    for k in (2, 3):
        one.trace_frames(10 + 3 * k, F, a_dev)
        assert np.array_equal(one.d2h(a_dev, (F, E, R)).view(np.uint32), grp.root.d2h(bufs[k & 1], (F, E, R)).view(np.uint32)), k
    grp.trace_frames(7, 1, bufs[0]); grp.synchronize(); one.trace_frames(7, 1, a_dev)       # one frame: the blocks land in place on device 0
    assert np.array_equal(one.d2h(a_dev, (1, E, R)).view(np.uint32), grp.root.d2h(bufs[0], (1, E, R)).view(np.uint32))
    one.free(a_dev); [grp.root.free(b) for b in bufs]
    grp.close(); one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,E,S,ranks", [("random1m", 256, 8192, 8), ("liver", 512, 16384, 8)])
def test_group_baseline_shapes_c4_c5(mcrt, tex256, name, E, S, ranks):
    """BASELINE C4 ("1 M random triangles, 256 x 8192 rays, scan-lines sharded across 2/4/8 GPUs with a gather") and C5 ("512 x 16384 rays + PSF
    convolution at 8 GPUs") as a SYSTEM: an eight-rank mcrt_group -- eight tracing contexts with their own scene copies and work buffers, eight
    host threads, eight peer copies, the root's post-processing; the ranks share the one GPU of the test box -- against one context tracing the
    whole frame: RF image and the PSF-convolved, enveloped, scan-converted B-mode frame bit for bit.  (That the single context's frame is the
    oracle's: tests/test_gpu_baseline_configs.py.)"""
    cfg, meshes = (mcrt.synth.random_scene(1_000_000, 8, 12345) if name == "random1m" else mcrt.synth.liver_scene(5))
    sd = mcrt.scene_io.build_scene(cfg, meshes)
    tr = mcrt.Transducer(E, position=cfg["transducerPosition"], angles_deg=cfg["transducerAngles"])
    psf = mcrt.Psf(freq=tr.frequency)
    frame = 1 if name == "random1m" else 7
    out = {}
    for who in ("one", "group"):
        obj = mcrt.Context(0) if who == "one" else mcrt.Group([0] * ranks)
        import time
        t0 = time.perf_counter()
        _setup(obj, mcrt, sd, tr, S, tex256)
        if who == "group":       # (one host build + eight uploads, not eight builds)
            print("\n%s: group of %d set up in %.2f s: host SAH build %.2f s (once), the ranks' uploads %.2f s (concurrent)" % ((name, ranks, time.perf_counter() - t0) + obj.last_scene_seconds()))
        else:
            print("\n%s: one context set up in %.2f s" % (name, time.perf_counter() - t0))
        root = obj if who == "one" else obj.root
        R = root.params.n_rows
        dev, img = root.alloc(E * R * 4), root.alloc(400 * 500 * 4)
        if who == "one":
            obj.trace_frames(frame, 1, dev)
        else:
            obj.trace_frames(frame, 1, dev)
            assert [mcrt.shard_range(r, ranks, E) for r in range(ranks)][-1][1] == E
        obj.synchronize()
        rf = root.d2h(dev, (E, R)).copy()
        root.convolve_frames(dev, 1, E, R, psf.axial_kernel, psf.lateral_kernel)
        root.envelope_frames(dev, 1, E, R)
        root.scan_convert_frames(dev, 1, E, R, img)
        obj.synchronize()
        out[who] = (rf, root.d2h(img, (400, 500)).copy())
        root.free(dev); root.free(img)
        obj.close()
    assert np.array_equal(out["one"][0].view(np.uint32), out["group"][0].view(np.uint32)) and np.nansum(np.abs(out["one"][0])) > 0
    assert np.array_equal(out["one"][1].view(np.uint32), out["group"][1].view(np.uint32)) and np.nansum(np.abs(out["one"][1])) > 0
