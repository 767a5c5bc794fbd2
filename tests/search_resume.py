"""What the GPU tests of the three backbones share to pin a resumed search: N iterations in one call against
N1 + N2 iterations continued through the returned `state` (first_step = steps done + 1), bit for bit."""
import torch


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def check_resumed_search(search, raw0, N, N1):
    """search(raw, n, state) -> (traj [n,b,.], (exp_avg, exp_avg_sq, steps_done)) runs n iterations on raw in place.

    First two identical one-shot runs of N iterations must be bit-equal (otherwise the loop is not run-to-run
    deterministic, and that is the finding).  Then N1 + (N - N1) iterations through `state` must give the one-shot
    run's raw mask, exp_avg, exp_avg_sq and trajectory rows bit for bit.  Last, the comparison can see what it is
    there for: the same continuation with the step count dropped from the state (Adam's bias correction restarted,
    and for the TF plan eps_hat too) must NOT reproduce the one-shot run."""
    def run(parts, forget_steps=False):
        raw, state, rows = raw0.clone(), None, []
        for n in parts:
            if state is not None and forget_steps:
                state = (state[0], state[1], 0)
            traj, state = search(raw, n, state)
            rows.append(traj)
        torch.cuda.synchronize()
        return (raw, state[0], state[1], torch.cat(rows, 0)), state[2]

    one, done = run([N])
    again, _ = run([N])
    assert done == N and one[3].shape[0] == N
    assert _same(one, again), "two identical one-shot searches differ: the loop is not run-to-run deterministic"
    split, done = run([N1, N - N1])
    assert done == N
    for name, p, q in zip(("raw_mask", "exp_avg", "exp_avg_sq", "trajectory"), one, split):
        assert torch.equal(_bits(p), _bits(q)), f"{name} of the resumed search differs from the one-shot search"
    restarted, _ = run([N1, N - N1], forget_steps=True)
    assert not torch.equal(_bits(one[0]), _bits(restarted[0]))
