"""Multi-GPU sharding of the hot path (one process per GPU, torch.distributed; backend "nccl" = RCCL over
xGMI on the MI355X node, "gloo" in the CPU tests).

The path is embarrassingly parallel: rays never interact, grid voxels never interact,
weights (2.4 MB / network) are replicated.  So there is NO collective inside the data path; each rank renders
a contiguous range of rays / axis-0 slab of the grid, and ONE all-gather at the end assembles the pixels, or the
emitted triangles of the per-slab marching cubes (`marching_cubes_sharded`: vertex ownership follows the global
plane index, so the ranks' arrays concatenated in rank order ARE the single-GPU mesh, vertex numbering included),
or -- `density_grid_sharded`, kept as the cross-check -- the density grid itself.
"""
import torch


def _dist():
    import torch.distributed as dist
    return dist


def world():
    dist = _dist()
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init_from_env(backend=None):
    """Join the process group a `torch.distributed.run` launcher describes through RANK / LOCAL_RANK /
    WORLD_SIZE (the reference's only multi-GPU hook is `Trainer(gpus=...)`, /root/reference/src/train_nerf.py:35-37,79;
    here the scripts are launched one process per GPU).  Binds this process to its GPU, initialises RCCL
    (backend "nccl") -- or `backend` when given, e.g. "gloo" in the CPU tests -- and returns (rank, world, device).
    Without a launcher environment it is a no-op returning (0, 1, current device).

    `NERFMESHES_RANKS_PER_GPU=k` (k > 1) puts k consecutive local ranks on the same GPU: a functional mode for
    exercising the N-rank code paths with the real kernels on a box with fewer GPUs than ranks.  RCCL refuses two ranks
    on one device, so that mode uses the "gloo" backend (device tensors staged through the host, `_via_host`); it says
    nothing about scaling."""
    import os
    dist = _dist()
    have_gpu = torch.cuda.is_available()
    if "WORLD_SIZE" not in os.environ or not dist.is_available():
        return 0, 1, torch.device("cuda", torch.cuda.current_device()) if have_gpu else torch.device("cpu")
    rank, ws = int(os.environ.get("RANK", "0")), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    per_gpu = max(1, int(os.environ.get("NERFMESHES_RANKS_PER_GPU", "1")))
    backend = backend or ("nccl" if have_gpu and per_gpu == 1 else "gloo")
    if per_gpu > 1 and backend == "nccl":
        raise RuntimeError("NERFMESHES_RANKS_PER_GPU > 1 needs the gloo backend: RCCL refuses duplicate devices")
    device = torch.device("cpu")
    if have_gpu:
        index = local // per_gpu
        if index >= torch.cuda.device_count():
            raise RuntimeError(f"LOCAL_RANK={local} ({per_gpu} rank(s) per GPU) but only {torch.cuda.device_count()} GPU(s) are visible")
        torch.cuda.set_device(index)
        device = torch.device("cuda", index)
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        kw = {"device_id": device} if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=ws, **kw)
    return rank, ws, device


def shutdown():
    dist = _dist()
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()


COLLECTIVES = {"count": 0}     # collectives issued by this module since import (tests and bench.py report the count per object)
PADDED_GATHER_LIMIT = 1 << 30   # bytes of world x max(counts) rows up to which a ragged gather is ONE padded collective


def _count():
    COLLECTIVES["count"] += 1


def _debug():
    import os
    return os.environ.get("NERFMESHES_DIST_DEBUG", "") not in ("", "0")


def _via_host(t):
    """True when a collective on `t` has to be staged through host memory: a device tensor under the gloo backend."""
    return t.is_cuda and _dist().get_backend() == "gloo"


def all_gather_into(out, local):
    """`dist.all_gather_into_tensor(out, local)`; device tensors under gloo go through the host."""
    dist = _dist()
    _count()
    if _via_host(local):
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, local.cpu().contiguous())
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, local.contiguous())
    return out


def all_reduce(t, op=None):
    dist = _dist()
    op = op if op is not None else dist.ReduceOp.SUM
    _count()
    if _via_host(t):
        host = t.cpu()
        dist.all_reduce(host, op=op)
        t.copy_(host)
    else:
        dist.all_reduce(t, op=op)
    return t


def broadcast(t, src=0):
    """`dist.broadcast(t, src)` in place; device tensors under gloo go through the host."""
    dist = _dist()
    _count()
    if _via_host(t):
        host = t.cpu()
        dist.broadcast(host, src=src)
        t.copy_(host)
    else:
        dist.broadcast(t, src=src)
    return t


def round_robin_counts(n, world_size):
    """Items per rank when item i goes to rank i % world_size."""
    return [len(range(r, n, world_size)) for r in range(world_size)]


def split_range(n, rank, world_size):
    """Contiguous near-equal split of range(n): the first n % world ranks get one extra item."""
    base, extra = divmod(n, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def own_range(n):
    """`split_range` for the current rank and world: (lo, hi, counts) -- this rank's part [lo, hi) of range(n) and every
    rank's item count, which is what `all_gather_rows` takes for the parts."""
    rank, ws = world()
    counts = [b - a for a, b in (split_range(n, r, ws) for r in range(ws))]
    return (*split_range(n, rank, ws), counts)


def slab_range(n0, rank, world_size):
    """Axis-0 planes of the density grid owned by `rank` (axis 0 is the outermost marching-cubes scan axis)."""
    return split_range(n0, rank, world_size)


def all_gather_rows(local, counts):
    """All-gather a ragged first dimension: `local` is this rank's (counts[rank], ...) tensor; returns the
    concatenation over ranks on every rank.  ONE collective either way: equal shards are all_gather_into_tensor
    straight into the result (one RCCL ring over xGMI); ragged shards travel padded to the largest one
    (`all_gather_v`) and are compacted on the device."""
    dist = _dist()
    rank, ws = world()
    if not (dist.is_available() and dist.is_initialized()):
        return local
    # an initialised group of ONE rank still goes through the collective (a device copy): the single-GPU
    # tests and `bench.py` exercise the same RCCL entry point the 8-GPU run uses
    if len(counts) != ws or counts[rank] != local.shape[0]:
        raise ValueError(f"all_gather_rows: rank {rank} holds {local.shape[0]} rows, counts = {list(counts)}")
    if _debug():
        check_counts(counts)
    tail = tuple(local.shape[1:])
    if len(set(counts)) == 1:
        out = torch.empty((sum(counts),) + tail, dtype=local.dtype, device=local.device)
        return all_gather_into(out, local)
    return all_gather_v(local, counts)


def check_counts(counts):
    """Debug aid (NERFMESHES_DIST_DEBUG=1): every rank must present the same `counts` to a ragged gather -- ranks that
    disagree would otherwise size their buffers differently and hang or corrupt the collective.  One extra all-gather."""
    rank, ws = world()
    mine = torch.tensor(list(counts), dtype=torch.int64)
    every = torch.empty(ws * len(counts), dtype=torch.int64)
    dev = torch.device("cuda", torch.cuda.current_device()) if _dist().get_backend() == "nccl" else torch.device("cpu")
    every = all_gather_into(every.to(dev), mine.to(dev)).cpu().view(ws, -1)
    if not bool((every == every[0]).all()):
        raise RuntimeError(f"ragged gather: the ranks disagree about the shard sizes: {every.tolist()}")


def all_gather_v(local, counts):
    """The ragged case of `all_gather_rows` as ONE collective: every rank contributes max(counts) rows (its own, padded),
    all_gather_into_tensor assembles (world, max, ...) and the shards are compacted into the exact-size result by one
    device-side concatenation.  At this path's sizes the padding is noise (triangles of a 480^3 mesh at 8 ranks: 8 x 9 MB
    instead of 40 MB, 0.5 ms of xGMI time) while a broadcast per rank -- round 4's exact-size form -- costs `world`
    latency-bound collectives; that form is kept for payloads beyond PADDED_GATHER_LIMIT.  Same calls under RCCL and gloo;
    device tensors under gloo are staged through the host."""
    dist = _dist()
    rank, ws = world()
    tail = tuple(local.shape[1:])
    row = local.element_size()
    for d in tail:
        row *= d
    mx, total = max(counts), sum(counts)
    if ws * mx * row <= PADDED_GATHER_LIMIT:
        send = torch.empty((mx,) + tail, dtype=local.dtype, device=local.device)
        send[:counts[rank]].copy_(local)
        buf = torch.empty((ws * mx,) + tail, dtype=local.dtype, device=local.device)
        all_gather_into(buf, send)
        buf = buf.view((ws, mx) + tail)
        return torch.cat([buf[r, :counts[r]] for r in range(ws) if counts[r]], dim=0) if total else buf[0, :0]
    host = _via_host(local)
    out = torch.empty((total,) + tail, dtype=local.dtype, device="cpu" if host else local.device)
    lo = 0
    for r in range(ws):
        hi = lo + counts[r]
        if hi > lo:
            piece = out[lo:hi]
            if r == rank:
                piece.copy_(local)
            _count()
            dist.broadcast(piece, src=r)
        lo = hi
    return out.to(local.device) if host else out


def render_view_sharded(render_fn, num_rays):
    """Each rank renders rays [lo, hi) with `render_fn(lo, hi) -> (hi-lo, C)` and all ranks receive the
    full (num_rays, C) image."""
    lo, hi, counts = own_range(num_rays)
    return all_gather_rows(render_fn(lo, hi), counts)


def density_grid_sharded(query_fn, n0, n1, n2):
    """Each rank evaluates its slab of axis-0 planes with `query_fn(plane_lo, plane_hi) -> ((hi-lo)*n1*n2,)`
    and all ranks receive the full (n0, n1, n2) grid."""
    lo, hi, counts = own_range(n0)
    return all_gather_rows(query_fn(lo, hi), [c * n1 * n2 for c in counts]).view(n0, n1, n2)


def all_gather_ragged(local):
    """All-gather of tensors whose first dimension differs per rank (the counts travel first)."""
    rank, ws = world()
    if ws == 1:
        return local
    mine = torch.tensor([local.shape[0]], dtype=torch.int64, device=local.device)
    counts = torch.empty(ws, dtype=torch.int64, device=local.device)
    all_gather_into(counts, mine)
    return all_gather_rows(local, [int(c) for c in counts.tolist()])


def slab_layers(n0, rank, world_size):
    """Marching cubes per slab: the cube layers [lo, hi) of rank `rank` (the n0 - 1 layers split like any range), whether
    a ghost layer below / above goes with them, and the voxel planes [p_lo, p_hi) it needs for that."""
    lo, hi = split_range(n0 - 1, rank, world_size)
    below, above = int(lo > 0 and hi > lo), int(hi < n0 - 1 and hi > lo)
    return lo, hi, below, above, lo - below, hi + 1 + above


def marching_cubes_sharded(query_fn, n0, n1, n2, iso_fn, refine=None):
    """Mesh of an (n0, n1, n2) density grid without assembling the grid anywhere (BASELINE north_star: "all-gather of ...
    emitted triangles"; replaces the grid all-gather in front of marching cubes, /root/reference/src/mesh_nerf.py:73-79).
    Rank r evaluates the planes of its own cube layers plus one ghost plane on either side -- `query_fn(p_lo, p_hi)` ->
    ((p_hi - p_lo) * n1 * n2,) densities; the 2 - 3 shared planes per boundary are recomputed rather than exchanged --,
    `iso_fn(slab, p_lo, own_lo, own_hi)` returns the iso level (collectively: numpy's statistics of the whole grid from
    per-rank chunk sums), every rank meshes its slab (nm_mc_count_slab / nm_mc_emit_slab: vertex ownership by GLOBAL plane
    index, vertex ids offset by the vertex counts of the lower ranks, which are all-gathered), and the four arrays travel
    in ONE all-gather of a packed byte buffer per rank: 2 collectives at any world size (+ 2 for a whole-grid iso level,
    `hip_ops.np_stats_sharded`).  The result equals the single-GPU mesh bit for bit, vertex numbering included.
    `refine(slab, p_lo, iso, verts, keys)` (optional) may move the slab's own vertices in place before they are packed (the
    super-sampled mesh: mesh_nerf.refine_vertices; keys = hip_ops.marching_cubes_slab's edge keys); None changes nothing.
    Returns (vertices, faces, normals, values, local slab (planes p_lo .. p_hi)).
    A mesh without a vertex is `hip_ops.marching_cubes`' two errors, with its texts and in its order: the gathered counts
    tell every rank, ONE more collective carries the minimum and maximum of every slab (on this path only), and all ranks
    raise together -- ValueError when the level lies outside the grid's range, else RuntimeError."""
    from . import hip_ops
    rank, ws = world()
    lo, hi, below, above, p_lo, p_hi = slab_layers(n0, rank, ws)
    plane = n1 * n2
    empty = hi == lo                          # more ranks than cube layers
    slab = query_fn(p_lo, p_hi).view(p_hi - p_lo, n1, n2) if not empty else None
    # voxel planes this rank accounts for in whole-grid statistics: its layers' lower planes; the last non-empty rank also
    # the top plane
    own_lo, own_hi = lo * plane, (hi + (1 if hi == n0 - 1 else 0)) * plane if not empty else lo * plane
    iso = iso_fn(slab, p_lo, own_lo, own_hi)
    dev = slab.device if slab is not None else torch.device("cuda", torch.cuda.current_device())
    # TWO collectives for the mesh whatever the world size: (vertices, faces) of every rank -- the vertex bases of the
    # ranks above need the counts below them --, then ONE gather of a byte buffer per rank that carries its four arrays
    # back to back (vertices | normals | values | faces: 28 V + 12 F bytes)
    piece = None if empty else hip_ops.marching_cubes_slab(slab, iso, p_lo, below, above)
    mine = torch.tensor([[0, 0] if empty else [piece.vertices, piece.faces]],        # the slab's OWN counts (ghost layer excluded)
                        dtype=torch.int64, device=dev)
    counts = torch.empty(ws, 2, dtype=torch.int64, device=dev)
    all_gather_into(counts, mine)
    counts = counts.cpu()
    # vertex ids of a slab are local id + (vertices of all lower slabs) - its ghost vertices (nm_mc_emit_slab)
    nv, nf = [int(c) for c in counts[:, 0]], [int(c) for c in counts[:, 1]]
    if sum(nv) == 0:
        # every rank sees the same counts, so all of them are here: the ends of every slab (its ghost planes are planes of the
        # grid; a rank without a slab contributes +inf / -inf) are those of the whole grid
        ends = torch.tensor([float("inf"), float("-inf")], device=dev) if empty else torch.stack(torch.aminmax(slab))
        ends = all_gather_into(torch.empty(ws, 2, dtype=torch.float32, device=dev), ends.view(1, 2))
        if iso < float(ends[:, 0].min()) or iso > float(ends[:, 1].max()):
            raise ValueError("Surface level must be within volume data range.")
        raise RuntimeError("No surface found at the given iso value.")
    if empty:
        payload = torch.empty(0, dtype=torch.uint8, device=dev)
    else:
        if refine is None:
            v, f, nrm, val = piece.emit(sum(nv[:rank]) - piece.ghost_vertices)       # (verts, faces, normals, values)
        else:
            v, f, nrm, val, keys = piece.emit(sum(nv[:rank]) - piece.ghost_vertices, return_keys=True)
            refine(slab, p_lo, iso, v, keys)
        payload = torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in (v, nrm, val, f)])
    # every rank's part ends in a 4-byte status word: a rank whose emit disagrees with the counts it announced still joins the
    # collective (with zeros of the promised size) -- raising before it would leave the other ranks inside the all-gather for
    # ever -- and ALL ranks raise together afterwards
    body = [28 * a + 12 * b for a, b in zip(nv, nf)]
    sizes = [b + 4 for b in body]
    bad = payload.numel() != body[rank]
    status = torch.tensor([payload.numel() if bad else -1], dtype=torch.int32, device=dev).view(torch.uint8)
    if bad:
        payload = torch.zeros(body[rank], dtype=torch.uint8, device=dev)
    flat = all_gather_rows(torch.cat([payload, status]), sizes)
    parts, lo, failed = ([], [], [], []), 0, []
    for r, (a, b) in enumerate(zip(nv, nf)):
        for k, (n_items, dtype) in enumerate(((3 * a, torch.float32), (3 * a, torch.float32), (a, torch.float32), (3 * b, torch.int32))):
            parts[k].append(flat[lo:lo + 4 * n_items].view(dtype))
            lo += 4 * n_items
        emitted = int(flat[lo:lo + 4].view(torch.int32).item())
        lo += 4
        if emitted != -1:
            failed.append(f"rank {r} emitted {emitted} bytes, its counts say {body[r]}")
    if failed:
        raise RuntimeError("marching_cubes_sharded: " + "; ".join(failed))
    vertices, normals, values, faces = (torch.cat(p) for p in parts)
    return vertices.view(-1, 3), faces.view(-1, 3), normals.view(-1, 3), values, slab


def all_reduce_gradients(parameters, bucket_bytes=64 << 20):
    """Data-parallel training: average the `.grad` of `parameters` over the ranks in
    place.  Every rank trains on its own ray batch; the two 8x256 networks have 1.19 M parameters = 4.8 MB, so
    ONE flat bucket (one RCCL ring all-reduce over xGMI, latency-bound at this size) carries them all; larger
    models are cut into `bucket_bytes` buckets.  Parameters without a gradient contribute zeros (every rank
    must present the same buckets)."""
    dist = _dist()
    rank, ws = world()
    params = [p for p in parameters if p.requires_grad]
    if ws == 1 or not params:
        return
    bucket, size = [], 0
    buckets = []
    for p in params:
        bucket.append(p)
        size += p.numel() * p.element_size()
        if size >= bucket_bytes:
            buckets.append(bucket)
            bucket, size = [], 0
    if bucket:
        buckets.append(bucket)
    for group in buckets:
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in group])
        all_reduce(flat, op=dist.ReduceOp.SUM)
        flat.div_(ws)
        offset = 0
        for p in group:
            n = p.numel()
            piece = flat[offset:offset + n].view_as(p)
            if p.grad is None:
                p.grad = piece.clone()
            else:
                p.grad.copy_(piece)
            offset += n
