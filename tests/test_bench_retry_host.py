"""CPU: the one retry tests/test_gpu_multirank.py allows a bench.py --mode tp run — for a death inside torch.distributed's own start-up, and for nothing else."""
from tests.test_gpu_multirank import _died_in_startup


def test_the_bench_retry_is_for_startup_deaths_only():
    """the retry used to fire on the exception's name anywhere in stderr; a crash after a leg or a marker line was printed must fail the caller's test"""
    boom = "terminate called after throwing an instance of 'std::bad_variant_access'\n"
    assert _died_in_startup(-6, "", boom) and _died_in_startup(134, "RCCL version 2.22\n", boom)
    assert not _died_in_startup(0, "", boom)                                                         # it did not fail
    assert not _died_in_startup(-6, "", "Segmentation fault\n")                                      # another death: reported
    assert not _died_in_startup(-6, '{"metric": "x"}\n', boom)                                       # a line came out first
    assert not _died_in_startup(-6, "", "[bench] leg native_plain failed: boom\n" + boom)            # a leg had run
    assert not _died_in_startup(-6, "", "[bench] rank 0: worker ended with status -6\n" + boom)      # the supervisor had a worker
