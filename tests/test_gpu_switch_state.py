"""Who owns the kernel-family switches around a fault (gesture2vec_amd.fault_policy, _lib.Context, csrc/misc.hip): the policy
puts back exactly what it switched off, the "already clear" notes that a switch voids are those of the context switched, and an
exception inside a Part d iteration does not leave the model deferring BatchNorm's running statistics.  No persistent or cluster
kernel is launched here: a pre-clear is a memset."""
import pytest
import torch

from gesture2vec_amd import _lib
from gesture2vec_amd._lib import Context
from gesture2vec_amd.fault_policy import PersistentPathPolicy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(ctx):
    return ctx.get(_lib.OPT_PERSISTENT), ctx.get(_lib.OPT_GRU_CLUSTER)


@pytest.fixture
def latch():
    """the library, with the process-wide fault latch clear before and after"""
    lib = _lib.load()
    lib.g2v_dec_rollout_persist_fault(1)
    yield lib
    lib.g2v_dec_rollout_persist_fault(1)


def test_policy_rearms_to_exactly_what_the_fault_switched_off(latch):
    ctx = Context()
    ctx.set(_lib.OPT_PERSISTENT, 2)
    ctx.set(_lib.OPT_GRU_CLUSTER, 0)
    pol = PersistentPathPolicy(rearm_after=3, max_rearms=1, ctx=ctx)
    latch.g2v_dec_rollout_persist_fault(-1)
    pol.on_fault()
    assert _pair(ctx) == (0, 0) and pol.off and latch.g2v_dec_rollout_persist_fault(0) == 0
    pol.on_fault()                                            # a further fault while off finds (0, 0): the first pair is kept
    assert pol._saved == (2, 0) and pol.off and pol.faults == 2
    assert [pol.tick(), pol.tick()] == [False, False] and _pair(ctx) == (0, 0)
    assert pol.tick() is True
    assert _pair(ctx) == (2, 0) and pol.rearms == 1 and not pol.off and pol.generation == 3
    assert _pair(Context.current()) == (1, 1)                 # (the default context was never touched)


def test_policy_has_nothing_to_rearm_when_both_families_were_off_already(latch):
    ctx = Context()
    ctx.set(_lib.OPT_PERSISTENT, 0)
    ctx.set(_lib.OPT_GRU_CLUSTER, 0)
    pol = PersistentPathPolicy(rearm_after=3, max_rearms=1, ctx=ctx)
    assert latch.g2v_dec_rollout_persist_fault(-1) == 1       # the latch set from the host, as a bounded wait running out would
    pol.on_fault()
    assert pol.off is False and pol.faults == 1 and pol.generation == 1
    assert [pol.tick() for _ in range(10)] == [False] * 10
    assert _pair(ctx) == (0, 0) and pol.rearms == 0
    assert latch.g2v_dec_rollout_persist_fault(0) == 0        # the latch was cleared all the same


def test_a_switch_voids_the_notes_of_the_context_that_was_switched(latch):
    lib = latch
    kind, T, B, D, H, ndir = 1, 20, 128, 40, 200, 2
    assert lib.g2v_gru_seq_cluster_ok(T, B, H, ndir) == 1     # (else the pre-clear below is a no-op and nothing is ever noted)
    ws = torch.empty(int(lib.g2v_gru_seq_bwd_workspace(ndir, H)), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    a, b = Context(), Context()
    notes = lambda ctx: ctx.get(_lib.OPT_PRECLEAR_NOTES)

    def note_in_a():
        with a:
            _lib.check(lib.g2v_cluster_exchange_preclear(kind, T, B, D, H, ndir, ws.data_ptr(), ws.numel(), st), "preclear")
        assert (notes(a), notes(b)) == (1, 0)

    with a:
        note_in_a()
        b.set(_lib.OPT_PERSISTENT, 1)                         # another context switched while A is bound: A's note stands
        assert (notes(a), notes(b)) == (1, 0)
    a.set(_lib.OPT_GRU_CLUSTER, 1)                            # A switched while nothing is bound: A's note is void
    assert notes(a) == 0
    note_in_a()
    PersistentPathPolicy(ctx=a).on_fault()                    # the engine-shaped route: the policy outside the binding
    assert notes(a) == 0 and _pair(a) == (0, 0)
    assert notes(b) == 0                                      # (B never held one)
    torch.cuda.synchronize()


def test_an_exception_inside_the_iteration_does_not_leave_batchnorm_deferred(monkeypatch):
    from test_gpu_text2embedding import _small_t2e
    from gesture2vec_amd.train_eval import train_seq2seq as TS
    args, net, optim, ids, lengths, codes, masks = _small_t2e(B=4, S=4)

    def boom(outputs, targets):
        raise RuntimeError("raised by the test behind the forward")
    monkeypatch.setattr(TS, "_code_loss_backward", boom)
    bn = net.decoder.decoder.pre_linear[1]
    with Context.current().scoped(persistent=0, gru_cluster=0):      # (the per-step kernels: what is tested is host bookkeeping)
        net.set_dropout_masks(*masks)
        with pytest.raises(RuntimeError, match="raised by the test"):
            TS.train_iter_text2embedding(args, 1, ids, lengths, None, None, codes, None, net, optim)
        assert net.deferred_bn is None
        mean0, nbt0 = bn.running_mean.detach().clone(), int(bn.num_batches_tracked)
        net.train()
        net.set_dropout_masks(*masks)
        net(ids, lengths, None, codes, None, None)            # a plain train-mode forward updates the statistics again
        torch.cuda.synchronize()
    assert not torch.equal(bn.running_mean, mean0), "the running mean stayed frozen"
    assert int(bn.num_batches_tracked) == nbt0 + codes.shape[1] - 1
