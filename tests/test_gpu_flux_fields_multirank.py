"""tpsrhs_surface_loads on a partitioned mesh, in the manner of tests/test_gpu_multirank.py: two ranks sharing the GPU (halo
exchange over torch.distributed / gloo) each reduce the wall faces they own, and the per-rank TOTAL loads add up to the
serial value within the surface header's own bound -- |error| <= K_s eps S per reduction (tests/surface_util.py), here the
serial reduction's plus each rank's, evaluated with the flux tensor each side actually integrated."""
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import surface_util as sfu
from tps_amd import capi, cases, meshgen
from tps_amd.rhs_operator import node_coordinates

pytestmark = pytest.mark.gpu
ORDER, WALL = 2, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    full = meshgen.scramble_orientations(meshgen.ogrid_cylinder(4, 12, 4), 21)
    ph = capi.dry_air_physics(capi.NS, visc_mult=2000.0)
    return full, ph, cases.cylinder_bcs(capi.VISC_ISOTH), cases.dry_air_state(node_coordinates(full, ORDER), seed=5)


def _loads_and_bound(op, mesh, x):
    """TOTAL loads of the wall patch, and K_s eps S of that reduction from the tensor that was integrated"""
    surf = op.createSurface(attributes=[WALL])
    loads = surf.loads(x, "total").cpu().numpy()
    F = op.getFlux(x, "total").cpu().numpy()  # [d][eq][n]
    surf.close()
    faces = capi.patch_faces(mesh, np.array([WALL], dtype=np.int32))
    ref = sfu.integrate(mesh, ORDER, 0, *faces, 1, np.ascontiguousarray(F.transpose(1, 0, 2)), sfu.FLUX, False)
    return loads[0], ref["K"][0] * sfu.EPS * ref["S"][0], int(faces[0].size)


def _worker(rank, world, port, q):
    try:
        import torch
        import torch.distributed as dist

        from tps_amd.halo import HaloExchange
        from tps_amd.rhs_operator import RHSoperator

        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        full, ph, bcs, Ug = _case()
        part = meshgen.partition(full, world, None)[rank]
        npe = (ORDER + 1) ** 3
        idx = (part.global_elements[:, None] * npe + np.arange(npe)[None, :]).ravel()
        op = RHSoperator(part, capi.Disc(ORDER, 0, 0, 0, 0), ph, bcs, device=0, halo=HaloExchange(device=torch.device("cuda", 0)))
        x = torch.tensor(np.ascontiguousarray(Ug[:, idx]).ravel(), dtype=torch.float64, device=op.device)
        loads, bound, nf = _loads_and_bound(op, part, x)
        dist.barrier()
        op.close()
        dist.destroy_process_group()
        q.put((rank, "ok", loads, bound, nf))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, traceback.format_exc(), None, None, None))


def test_rank_loads_add_up_to_the_serial_value():
    import torch

    from tps_amd.rhs_operator import RHSoperator

    world = 2
    full, ph, bcs, Ug = _case()
    op = RHSoperator(full, capi.Disc(ORDER, 0, 0, 0, 0), ph, bcs)
    x = torch.tensor(np.ascontiguousarray(Ug).ravel(), dtype=torch.float64, device=op.device)
    serial, bound, nf = _loads_and_bound(op, full, x)
    op.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:  # a rank that fails leaves its peer blocked in the exchange: collect what arrives, then end them all
        for _ in procs:
            res.append(q.get(timeout=300))
            if res[-1][1] != "ok":
                break
    finally:
        for p in procs:
            p.join(timeout=60 if len(res) == len(procs) and all(r[1] == "ok" for r in res) else 5)
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join()
    assert len(res) == len(procs), "a rank ended without reporting"
    total = np.zeros_like(serial)
    faces = 0
    for rank, msg, loads, b, n in res:
        assert msg == "ok", f"rank {rank}: {msg}"
        total += loads
        bound = bound + b
        faces += n
    assert faces == nf and all(r[4] > 0 for r in res), "every rank owns a part of the wall"
    err = np.abs(total - serial)
    print("sum of the rank loads - serial, as a fraction of the bound:", err / bound)
    assert np.all(np.abs(serial[1:]) > 0.0)
    assert np.all(err <= bound), (err, bound)
