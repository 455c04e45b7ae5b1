"""A context whose "chip-sized" grids are one compute unit's (MGX_GRID_CUS=1, include/mgx/env.hpp): num_cus * 8 workgroups are then
8, so on a small graph every wave runs its grid-stride loop many times -- the stages' carry-over from one iteration to the next
and every kernel's later iterations, which the session context reaches from about RMAT-20 on only."""
import contextlib


@contextlib.contextmanager
def one_cu_context(monkeypatch, torch):
    import mini_amd
    monkeypatch.setenv("MGX_GRID_CUS", "1")
    ctx = mini_amd.Context(0, torch.cuda.current_stream().cuda_stream)      # (the switch is read here, once)
    monkeypatch.delenv("MGX_GRID_CUS")
    try:
        assert ctx.num_cus == 1
        yield ctx
    finally:
        ctx.close()
