"""fork / join / SideStreams (basedet_amd/streams.py) on real streams: which stream is current inside and after a fork, and that a
join orders the side stream's work in front of the main stream's reads."""
import pytest
import torch

from basedet_amd.streams import SideStreams, fork, join

pytestmark = pytest.mark.gpu
N = 1 << 22
ADDS = 20


def test_fork_switches_the_current_stream_and_restores_it():
    main = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    with fork(s):
        assert torch.cuda.current_stream() == s
    assert torch.cuda.current_stream() == main
    with pytest.raises(KeyError, match="from the body"):
        with fork(s):
            assert torch.cuda.current_stream() == s
            raise KeyError("from the body")
    assert torch.cuda.current_stream() == main
    with fork(None):
        assert torch.cuda.current_stream() == main


def test_forks_nest_like_a_model_step_inside_the_solvers_stream():
    main = torch.cuda.current_stream()
    outer, inner = torch.cuda.Stream(priority=-1), torch.cuda.Stream()
    with fork(outer):
        with fork(inner):
            assert torch.cuda.current_stream() == inner
        assert torch.cuda.current_stream() == outer
        join(inner)
        assert torch.cuda.current_stream() == outer
    join(outer)
    assert torch.cuda.current_stream() == main


@pytest.mark.parametrize("wait", [True, False])
def test_fork_runs_behind_the_main_stream_and_join_in_front_of_it(wait):
    """wait=False with the wait written out by hand is the same fork."""
    s = torch.cuda.Stream()
    a = torch.empty(N, dtype=torch.float32, device="cuda")
    a.fill_(1.0)
    for _ in range(ADDS):
        a.add_(1)
    if not wait:
        s.wait_stream(torch.cuda.current_stream())
    with fork(s, wait=wait):
        b = a.clone()
    join(s)
    b.record_stream(torch.cuda.current_stream())          # (allocated on s, read here)
    assert int((b == 1.0 + ADDS).sum()) == N


def test_side_streams_are_two_and_join_all_waits_with_the_flag_off():
    st = SideStreams("cuda")
    assert st.wgrad_stream is not None and st.aux_stream is not None and st.wgrad_stream != st.aux_stream
    assert st.wgrad() == st.wgrad_stream and st.aux() == st.aux_stream
    a = torch.ones(N, dtype=torch.float32, device="cuda")
    out = []
    for s in (st.wgrad(), st.aux()):
        with fork(s):
            b = a.clone()
            for _ in range(ADDS):
                b.add_(1)
            out.append(b)
    st.enabled = False
    assert st.wgrad() is None and st.aux() is None
    st.join_all()                                           # the work enqueued above is still waited for
    for b in out:
        b.record_stream(torch.cuda.current_stream())
        assert int((b == 1.0 + ADDS).sum()) == N
