# Builds the product library udpdk_amd/libudpdk_amd.so (HIP kernels for gfx950 + C-ABI host code
# + the C udpdk_api.h host layer) and the test-only oracle (oracle/liboracle.so).
HIPCC     ?= /opt/rocm/bin/hipcc
CC        ?= gcc
ARCH      ?= gfx950
HIPFLAGS  ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Werror -Wno-unused-result
CFLAGS_H  ?= -O2 -std=gnu11 -fPIC -Wall -Wextra -Werror
INC       := -Iinclude -Iudpdk_amd/csrc
LIB       := udpdk_amd/libudpdk_amd.so
OBJDIR    := build/obj

HIP_SRC   := udpdk_amd/csrc/rx_classify.hip udpdk_amd/csrc/rx_lanes.hip udpdk_amd/csrc/rx_gather.hip udpdk_amd/csrc/rx_reasm.hip \
             udpdk_amd/csrc/rx_rss.hip udpdk_amd/csrc/tx_kernels.hip udpdk_amd/csrc/tx_reply.hip udpdk_amd/csrc/tx_segment.hip udpdk_amd/csrc/rx_filter.hip udpdk_amd/csrc/rx_balance.hip udpdk_amd/csrc/rx_peer.hip udpdk_amd/csrc/rx_mcast.hip udpdk_amd/csrc/icmp_reply.hip udpdk_amd/csrc/icmp_error.hip udpdk_amd/csrc/arp_reply.hip udpdk_amd/csrc/igmp_reply.hip udpdk_amd/csrc/neigh.hip udpdk_amd/csrc/udpdk_gpu_ctl.hip \
             udpdk_amd/csrc/udpdk_gpu.hip
C_SRC     := $(wildcard udpdk_amd/csrc/host/*.c)
HIP_OBJ   := $(patsubst udpdk_amd/csrc/%.hip,$(OBJDIR)/%.o,$(HIP_SRC))
C_OBJ     := $(patsubst udpdk_amd/csrc/host/%.c,$(OBJDIR)/host/%.o,$(C_SRC))
HDRS      := include/udpdk_gpu.h include/udpdk_api.h udpdk_amd/csrc/rx_common.h \
             udpdk_amd/csrc/rx_plan.h udpdk_amd/csrc/rx_filter.h udpdk_amd/csrc/rx_balance.h udpdk_amd/csrc/rx_peer.h udpdk_amd/csrc/rx_mcast.h udpdk_amd/csrc/icmp_reply.h udpdk_amd/csrc/icmp_error.h udpdk_amd/csrc/arp_reply.h udpdk_amd/csrc/igmp_reply.h udpdk_amd/csrc/neigh.h udpdk_amd/csrc/tx_ipv4.h udpdk_amd/csrc/lane_find.h udpdk_amd/csrc/rss_toeplitz.h udpdk_amd/csrc/rss_host.h udpdk_amd/csrc/wave.h udpdk_amd/csrc/fanin_stage.h udpdk_amd/csrc/gpu_ctx.h udpdk_amd/csrc/stamps.h $(wildcard udpdk_amd/csrc/host/*.h)

TOOLS     := tools/bin/bench_sock build/rx_plan_check build/rss_host_check build/echo_expand_check build/icmp_queue_check build/arp_frame_check build/igmp_frame_check

all: $(LIB) oracle $(TOOLS)

$(OBJDIR)/%.o: udpdk_amd/csrc/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) $(INC) -c $< -o $@

$(OBJDIR)/host/%.o: udpdk_amd/csrc/host/%.c $(HDRS)
	@mkdir -p $(dir $@)
	$(CC) $(CFLAGS_H) $(INC) -c $< -o $@

$(LIB): $(HIP_OBJ) $(C_OBJ) udpdk_amd/csrc/libudpdk_amd.map
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(HIP_OBJ) $(C_OBJ) -Wl,--no-undefined \
	    -Wl,-soname,libudpdk_amd.so -Wl,--version-script=udpdk_amd/csrc/libudpdk_amd.map

oracle: $(LIB)
	$(MAKE) -C oracle

# the reference-API path end to end, written against udpdk_api.h like a reference app (bench.py)
tools/bin/bench_sock: tools/bench_sock.c include/udpdk_api.h include/udpdk_gpu.h $(LIB)
	@mkdir -p tools/bin
	$(CC) -O2 -std=gnu11 -Wall -Wextra -Werror -Iinclude $< -o $@ -Ludpdk_amd -ludpdk_amd -Wl,-rpath,'$$ORIGIN/../../udpdk_amd'

# the RX launch planner behind a main(): host code only, links no project library and runs on a
# machine without a GPU (tests/test_rx_plan.py)
build/rx_plan_check: tools/rx_plan_check.cpp $(HDRS)
	@mkdir -p build
	$(HIPCC) -x hip --cuda-host-only -O1 -std=c++17 -Wall -Werror $(INC) $< -o $@

# the host's RSS table builder and per-frame hash behind a main(): host code only, links no project
# library and runs on a machine without a GPU (tests/test_rss_host.py); rss-asan builds the same
# program with the address and undefined-behaviour sanitizers (host only, never loaded into Python)
build/rss_host_check: tools/rss_host_check.c udpdk_amd/csrc/rss_host.h
	@mkdir -p build
	$(CC) -O1 -std=gnu11 -Wall -Wextra -Werror $(INC) $< -o $@
rss-asan: build/rss_host_check_asan
build/rss_host_check_asan: tools/rss_host_check.c udpdk_amd/csrc/rss_host.h
	@mkdir -p build
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all $(INC) $< -o $@

# udpdk_poll_echo's frame-table expansion behind a main(): host code only, links no project library
# and runs on a machine without a GPU (tests/test_tx_reply_ref.py); echo-asan builds the same
# program with the address and undefined-behaviour sanitizers (host only, never loaded into Python)
build/echo_expand_check: tools/echo_expand_check.c udpdk_amd/csrc/host/echo_expand.h
	@mkdir -p build
	$(CC) -O1 -std=gnu11 -Wall -Wextra -Werror $(INC) $< -o $@
echo-asan: build/echo_expand_check_asan
build/echo_expand_check_asan: tools/echo_expand_check.c udpdk_amd/csrc/host/echo_expand.h
	@mkdir -p build
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all $(INC) $< -o $@

# the host ICMP queue behind a main(): host code only, links no project library and runs on a machine
# without a GPU (tests/test_icmp_ref.py); icmp-asan builds the same program with the address and
# undefined-behaviour sanitizers (host only, never loaded into Python)
build/icmp_queue_check: tools/icmp_queue_check.c udpdk_amd/csrc/host/icmp_queue.h
	@mkdir -p build
	$(CC) -O1 -std=gnu11 -Wall -Wextra -Werror $(INC) $< -o $@
icmp-asan: build/icmp_queue_check_asan
build/icmp_queue_check_asan: tools/icmp_queue_check.c udpdk_amd/csrc/host/icmp_queue.h
	@mkdir -p build
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all $(INC) $< -o $@

# the host's ARP announcement builder behind a main(): host code only, links no project library and
# runs on a machine without a GPU (tests/test_arp_ref.py); arp-asan builds the same program with the
# address and undefined-behaviour sanitizers (host only, never loaded into Python)
build/arp_frame_check: tools/arp_frame_check.c udpdk_amd/csrc/host/arp_frame.h
	@mkdir -p build
	$(CC) -O1 -std=gnu11 -Wall -Wextra -Werror $(INC) $< -o $@
arp-asan: build/arp_frame_check_asan
build/arp_frame_check_asan: tools/arp_frame_check.c udpdk_amd/csrc/host/arp_frame.h
	@mkdir -p build
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all $(INC) $< -o $@

# the host's IGMP report and leave builder behind a main(): host code only, links no project library
# and runs on a machine without a GPU (tests/test_mcast_ref.py); igmp-asan builds the same program with
# the address and undefined-behaviour sanitizers (host only, never loaded into Python)
build/igmp_frame_check: tools/igmp_frame_check.c udpdk_amd/csrc/host/igmp_frame.h
	@mkdir -p build
	$(CC) -O1 -std=gnu11 -Wall -Wextra -Werror $(INC) $< -o $@
igmp-asan: build/igmp_frame_check_asan
build/igmp_frame_check_asan: tools/igmp_frame_check.c udpdk_amd/csrc/host/igmp_frame.h
	@mkdir -p build
	$(CC) -O1 -g -std=gnu11 -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all $(INC) $< -o $@

# diagnostic library with per-phase s_memtime stamps (tools/stamps.py); never used by tests/bench
STAMP_LIB := tools/diag/libudpdk_amd.so
STAMP_OBJ := $(patsubst udpdk_amd/csrc/%.hip,build/stamps/%.o,$(HIP_SRC))
stamps: $(STAMP_LIB)
build/stamps/%.o: udpdk_amd/csrc/%.hip $(HDRS)
	@mkdir -p build/stamps
	$(HIPCC) $(HIPFLAGS) -DUDPDK_STAMPS $(INC) -c $< -o $@
$(STAMP_LIB): $(STAMP_OBJ) $(C_OBJ)
	@mkdir -p tools/diag
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -Wl,--no-undefined

# diagnostic library with per-phase wall-clock timing inside udpdk_poll_rx (tools/sock_prof.sh)
PROF_LIB := tools/diag/pollprof/libudpdk_amd.so
PROF_OBJ := $(patsubst udpdk_amd/csrc/host/%.c,build/pollprof/%.o,$(C_SRC))
pollprof: $(PROF_LIB)
build/pollprof/%.o: udpdk_amd/csrc/host/%.c $(HDRS)
	@mkdir -p build/pollprof
	$(CC) $(CFLAGS_H) -DUDPDK_POLL_PROFILE $(INC) -c $< -o $@
$(PROF_LIB): $(HIP_OBJ) $(PROF_OBJ)
	@mkdir -p tools/diag/pollprof
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -Wl,--no-undefined -Wl,-soname,libudpdk_amd.so

# A/B variant of the library (tools/ab.py): `make variant VAR=name VFLAGS="-DX=1"` builds
# tools/var/name.so from the same sources with extra compile flags; never used by tests/bench
VAR       ?= new
VFLAGS    ?=
VAR_OBJ   := $(patsubst udpdk_amd/csrc/%.hip,build/var/$(VAR)/%.o,$(HIP_SRC)) \
             $(patsubst udpdk_amd/csrc/host/%.c,build/var/$(VAR)/host/%.o,$(C_SRC))
variant: tools/var/$(VAR).so
build/var/$(VAR)/%.o: udpdk_amd/csrc/%.hip $(HDRS) FORCE
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) $(VFLAGS) $(INC) -c $< -o $@
build/var/$(VAR)/host/%.o: udpdk_amd/csrc/host/%.c $(HDRS) FORCE
	@mkdir -p $(dir $@)
	$(CC) $(CFLAGS_H) $(VFLAGS) $(INC) -c $< -o $@
tools/var/$(VAR).so: $(VAR_OBJ)
	@mkdir -p tools/var
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $^ -Wl,--no-undefined \
	    -Wl,-soname,libudpdk_amd.so -Wl,--version-script=udpdk_amd/csrc/libudpdk_amd.map
FORCE:

# device assembly and the resource-usage report of every HIP source: build/asm/<file>.s,
# build/asm/<file>_resource.txt (tools/diag/asm_stats.py reads the .s)
ASM_OUT   := $(patsubst udpdk_amd/csrc/%.hip,build/asm/%.s,$(HIP_SRC))
asm: $(ASM_OUT)
build/asm/%.s: udpdk_amd/csrc/%.hip $(HDRS)
	@mkdir -p build/asm
	$(HIPCC) $(HIPFLAGS) -Wno-unused-command-line-argument $(INC) -S --cuda-device-only -o $@ $<
	$(HIPCC) $(HIPFLAGS) $(INC) -c -Rpass-analysis=kernel-resource-usage $< -o /dev/null 2> build/asm/$*_resource.txt || true

clean:
	rm -rf build $(LIB) $(TOOLS)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean asm stamps pollprof variant rss-asan echo-asan icmp-asan arp-asan igmp-asan FORCE
