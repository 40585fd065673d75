# The sources that compile without HIP, and the flags every build of them shares.  This is what a CPU build links: the library's Makefile
# takes it as the front of HOSTSRC, tests/san/Makefile and tests/host_build.py (the stand-alone check programs) build exactly this list.
# Keep each assignment on one line: host_build.py reads them as text.
HOSTONLY_SRC = hash.cpp hostfast.cpp hostifma.cpp hostgroup.cpp spartan_host.cpp wire.cpp snark_host.cpp zkif.cpp
HOSTONLY_WARN = -Wall -Wno-unused-function
HOSTONLY_ARCH = -march=x86-64-v3
