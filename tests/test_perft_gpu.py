"""GPU tests of perft on the MI355X: the published counts at every listed depth and three deeper trees, each at the default capacity
and at one that splits at least two levels; the move statistics and the ORDER checksum at depth 4 against the walk over the oracle;
the device against the wave emulator; two calls on two streams."""
import threading

import pytest
import torch

import perft_cases as PC
from betaone_amd import perft as P
from test_oracle_rules import PERFT

pytestmark = pytest.mark.gpu

DEEP = [(PC.START, 6, 119060324, 197281), (PC.KIWIPETE, 5, 193690690, 97862), (PC.POS3, 6, 11030083, 43238)]  # fen, depth, perft(depth), perft(depth - 2)


def split_capacity(below):
    """A capacity that splits the last TWO expansions of a walk to depth D: `below` = perft(D - 2) positions of level D - 2 do not fit
    a buffer of half as many (so the level above is expanded in chunks), and level D - 1 is larger still."""
    cap = max(P.MIN_CAPACITY, below // 2)
    assert cap < below
    return cap


@pytest.mark.parametrize("fen,expected", PERFT)
def test_published_counts_at_every_listed_depth(fen, expected):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    PC.check_counts_and_divide("hip", fen, expected, range(1, len(expected) + 1))
    for d in range(3, len(expected) + 1):
        if expected[d - 3] > P.MIN_CAPACITY:
            whole = PC.run("hip", fen, d, divide=True)
            split = PC.run("hip", fen, d, divide=True, capacity=split_capacity(expected[d - 3]))
            assert whole.splits == 0 and split.splits >= 2, (fen, d, split.splits)
            PC.same_result(split, whole)


@pytest.mark.parametrize("fen,depth,nodes,below", DEEP)
def test_deep_counts(fen, depth, nodes, below):
    whole = PC.run("hip", fen, depth, divide=True)
    print(f"{fen} depth {depth}: {whole.nodes} nodes in {whole.seconds:.3f} s")
    assert whole.nodes == nodes and whole.splits == 0 and sum(n for _, n in whole.moves) == nodes
    split = PC.run("hip", fen, depth, divide=True, capacity=split_capacity(below))
    assert split.splits >= 2
    PC.same_result(split, whole)


@pytest.mark.parametrize("fen", [PC.KIWIPETE, PC.POS5])
def test_stats_and_order_checksum_at_depth_4(fen):
    PC.check_stats_and_order("hip", fen, 4)


@pytest.mark.parametrize("fen", PC.STATS_FENS)
def test_device_equals_emulator_on_the_depth_3_cases(fen):
    PC.same_result(PC.run("hip", fen, 3, divide=True, stats=True, order=True), PC.run("emu", fen, 3, divide=True, stats=True, order=True))


@pytest.mark.parametrize("fen,expected", PERFT)
def test_device_equals_emulator_counts_at_depth_3(fen, expected):
    PC.same_result(PC.run("hip", fen, 3, divide=True, order=True), PC.run("emu", fen, 3, divide=True, order=True))


def test_two_calls_on_two_streams():
    jobs = [(PC.KIWIPETE, 4), (PC.START, 5)]
    alone = [P.perft(f, d, divide=True, stats=True, order=True)[0] for f, d in jobs]
    got = [None, None]

    def work(i):
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):
            got[i] = P.perft(jobs[i][0], jobs[i][1], divide=True, stats=True, order=True)[0]

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for a, b in zip(alone, got):
        assert b is not None
        PC.same_result(a, b)
    assert alone[0].nodes == PERFT[1][1][3] and alone[1].nodes == PERFT[0][1][4]
