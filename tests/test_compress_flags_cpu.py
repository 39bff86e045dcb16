"""CPU: --compress / --compression-level of `python -m msweep_amd` are judged before a device is touched -- bz2, lzma,
zstd and anything else are refused in the reference's words (src/OutfileDesignator.cpp:30-62), a level outside 0 ... 9
likewise, exit status 1."""
import pytest

from msweep_amd import __main__ as cli


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the refusal must come before the GPU is initialised")
    monkeypatch.setattr(cli, "Core", boom)


@pytest.mark.parametrize("kind", ["bz2", "lzma", "zstd", "gzip", ""])
def test_other_compression_types_are_refused(no_device, capsys, tmp_path, kind):
    rc = cli.main(["-i", str(tmp_path / "none.txt"), "--themisto-1", "a", "-o", str(tmp_path / "o"), "--write-probs", "--compress", kind])
    err = capsys.readouterr().err
    assert rc == 1
    assert f"unsupported compression type {kind}" in err and "z only" in err


@pytest.mark.parametrize("level", ["10", "-1", "99"])
def test_levels_outside_0_to_9_are_refused(no_device, capsys, tmp_path, level):
    rc = cli.main(["-i", str(tmp_path / "none.txt"), "--themisto-1", "a", "-o", str(tmp_path / "o"), "--compress", "z",
                   "--compression-level", level])
    err = capsys.readouterr().err
    assert rc == 1
    assert f"unsupported compression level {level}" in err and "z only" in err


def test_valid_flags_pass_the_check(monkeypatch, tmp_path):
    """plaintext, z and every level 0 ... 9 get as far as the device"""
    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(cli, "Core", reached)
    for extra in (["--compress", "plaintext"], ["--compress", "z"], ["--compress", "z", "--compression-level", "0"],
                  ["--compress", "z", "--compression-level", "9"], []):
        with pytest.raises(Reached):
            cli.main(["-i", str(tmp_path / "none.txt"), "--themisto-1", "a", "-o", str(tmp_path / "o")] + extra)
