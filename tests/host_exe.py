"""The build step of every test that runs a program of composable_sdr_amd/host."""
import os
import subprocess

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "composable_sdr_amd", "host")


def host_exe(name):
    """The path of the host program `name`, brought up to date first: make, not the file's mere existence, decides whether it
    is stale (a binary older than csdr_host.hpp would otherwise pass the test on old code)."""
    subprocess.check_call(["make", "-C", HOST, "-s", name])
    return os.path.join(HOST, name)
