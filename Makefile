# fantoch_amd build (no cmake/ninja needed).  `make` builds the product
# library and the oracle; both are plain in-tree .so files so they travel to
# the GPU box with the repo snapshot.
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
ARCH ?= gfx950
JOBS ?= 8

LIB := fantoch_amd/libfantoch_amd.so
ORACLE := oracle/build/liboracle.so
CPPTEST := tests/cpp/build/test_graph_executor

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function \
            -Iinclude -Ifantoch_amd/csrc -mllvm -simplifycfg-sink-common=false
SRCS := fantoch_amd/csrc/fx_ladder.hip fantoch_amd/csrc/fx_runtime.hip fantoch_amd/csrc/graph_tiers.hip fantoch_amd/csrc/graph_exec.hip fantoch_amd/csrc/graph_metrics.hip fantoch_amd/csrc/metrics_host.cpp fantoch_amd/csrc/graph_synth.hip fantoch_amd/csrc/handle_xfer.hip fantoch_amd/csrc/graph_group.hip fantoch_amd/csrc/graph_wave.hip fantoch_amd/csrc/graph_lane.hip fantoch_amd/csrc/graph_split.hip fantoch_amd/csrc/graph_cut.hip fantoch_amd/csrc/graph_wide.hip fantoch_amd/csrc/pred_exec.hip fantoch_amd/csrc/pred_advance.hip fantoch_amd/csrc/pred_host.cpp fantoch_amd/csrc/pred_synth.hip fantoch_amd/csrc/pred_synth_host.cpp fantoch_amd/csrc/table_exec.hip fantoch_amd/csrc/table_synth.hip fantoch_amd/csrc/table_group_synth.hip fantoch_amd/csrc/table_synth_host.cpp fantoch_amd/csrc/kv_exec.hip fantoch_amd/csrc/kv_advance.hip fantoch_amd/csrc/kv_host.cpp fantoch_amd/csrc/pending_exec.hip fantoch_amd/csrc/pending_advance.hip fantoch_amd/csrc/pending_host.cpp fantoch_amd/csrc/slot_exec.hip fantoch_amd/csrc/slot_advance.hip fantoch_amd/csrc/slot_host.cpp fantoch_amd/csrc/executor_host.cpp fantoch_amd/csrc/exec_log.cpp fantoch_amd/csrc/config.cpp fantoch_amd/csrc/planet.cpp fantoch_amd/csrc/sim_wave.hip fantoch_amd/csrc/sim_big.hip
HDRS := include/fantoch_amd.h include/fantoch_amd.hpp fantoch_amd/csrc/fx_synth.h fantoch_amd/csrc/fx_table_synth.h fantoch_amd/csrc/fx_table_group_synth.h fantoch_amd/csrc/fx_kv.h fantoch_amd/csrc/fx_pending.h fantoch_amd/csrc/fx_slot.h fantoch_amd/csrc/fx_pred.h fantoch_amd/csrc/fx_pred_synth.h fantoch_amd/csrc/fx_metrics.h fantoch_amd/csrc/fx_internal.h fantoch_amd/csrc/fx_wave.h fantoch_amd/csrc/table_window.h fantoch_amd/csrc/table_state.h fantoch_amd/csrc/table_event.inc fantoch_amd/csrc/table_wave.inc fantoch_amd/csrc/kv_step.inc fantoch_amd/csrc/pending_step.inc

POISON := tests/poison/build/libpoison.so
HLAT := tools/build/handle_latency

all: $(LIB) $(ORACLE) $(CPPTEST) $(POISON) $(HLAT)

# one object per source (make -j compiles them in parallel), then one link
OBJDIR := fantoch_amd/build/obj
OBJS := $(patsubst fantoch_amd/csrc/%,$(OBJDIR)/%.o,$(SRCS))
$(OBJDIR)/%.o: fantoch_amd/csrc/% $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# k_sim under the iterative ILP scheduler: configs[1] 425.8 -> 430.0 M
# (round 4, tools/sim_ab.sh).  Round 3 could not adopt it: its n = 7 build
# stopped with FX_ERR_SIM_LATE, because prm()'s inline v_readlane lacked the
# one wait state a VALU write of the same VGPR needs (sim_wave.hip prm, fixed
# in round 4; tests/test_sim_poison.py's zero fill catches it deterministically).
# max-ilp / min-reg / max-occupancy / memory-clause: 418 - 423 M (round 3).
# Round 6, same box, two runs each (profiles/r06_sim_sched_ab.txt): iterative-ILP
# 428.9 / 429.2 / 429.6 M; max-ilp 430.1 / 430.4 / 429.9; iterative-ILP with
# -amdgpu-set-wave-priority 431.5 / 431.0 / 429.8; max-ilp with it 427.2 / 426.9;
# iterative-minreg 428.6: within noise, so the schedule the tests ran on stays.
SIM_SCHED := -mllvm -amdgpu-sched-strategy=iterative-ilp
# the large-instance simulator and the wide executor tiers under the iterative
# ILP scheduler: configs[3] simulator 99.1 -> 103.1 M, dense executor 66.7 ->
# 68.0 M (tools/mode_ab.sh), every GPU test passing
$(OBJDIR)/sim_big.hip.o $(OBJDIR)/graph_wide.hip.o $(OBJDIR)/sim_wave.hip.o: HIPFLAGS += -mllvm -amdgpu-sched-strategy=iterative-ilp

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS)

# phase-cycle profile build of the simulator (tools/sim_phase.py; FX_LIB=...)
PROF_LIB := fantoch_amd/build_prof/libfantoch_amd.so
prof: $(PROF_LIB)
$(PROF_LIB): $(SRCS) $(HDRS)
	@mkdir -p fantoch_amd/build_prof
	$(HIPCC) $(HIPFLAGS) $(SIM_SCHED) -DFX_SIM_PROFILE -shared -o $@ $(SRCS)

# measurement-only variants of the library (A/B and ablations, FX_LIB=...):
# make variant V=name D="-DFOO=1" rebuilds sim_wave.hip with the extra flags
# and links it with the other objects into fantoch_amd/build_$(V)/
variant: $(OBJS)
	@mkdir -p fantoch_amd/build_$(V)
	$(HIPCC) $(HIPFLAGS) $(SIM_SCHED) $(D) -c -o fantoch_amd/build_$(V)/sim_wave.o fantoch_amd/csrc/sim_wave.hip
	$(HIPCC) --offload-arch=$(ARCH) -shared -o fantoch_amd/build_$(V)/libfantoch_amd.so \
	  $(filter-out $(OBJDIR)/sim_wave.hip.o,$(OBJS)) fantoch_amd/build_$(V)/sim_wave.o

# the same for the wide executor tier (graph_wide.hip): make wvariant V=name D="-DFOO=1"
wvariant: $(OBJS)
	@mkdir -p fantoch_amd/build_$(V)
	$(HIPCC) $(HIPFLAGS) $(D) -c -o fantoch_amd/build_$(V)/graph_wide.o fantoch_amd/csrc/graph_wide.hip
	$(HIPCC) --offload-arch=$(ARCH) -shared -o fantoch_amd/build_$(V)/libfantoch_amd.so \
	  $(filter-out $(OBJDIR)/graph_wide.hip.o,$(OBJS)) fantoch_amd/build_$(V)/graph_wide.o

# any one source: make fvariant V=name F=sim_big D="-DFOO=1" (F = a .hip under csrc/)
fvariant: $(OBJS)
	@mkdir -p fantoch_amd/build_$(V)
	$(HIPCC) $(HIPFLAGS) $(D) -c -o fantoch_amd/build_$(V)/$(F).o fantoch_amd/csrc/$(F).hip
	$(HIPCC) --offload-arch=$(ARCH) -shared -o fantoch_amd/build_$(V)/libfantoch_amd.so \
	  $(filter-out $(OBJDIR)/$(F).hip.o,$(OBJS)) fantoch_amd/build_$(V)/$(F).o

ORACLE_SRCS := oracle/graph_oracle.cpp oracle/sim_oracle.cpp oracle/pred_oracle.cpp
$(ORACLE): $(ORACLE_SRCS) oracle/graph_oracle.hpp include/fantoch_amd.h
	@mkdir -p oracle/build
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -o $@ $(ORACLE_SRCS) -lpthread

# C++ port of the reference's graph unit tests against the C++ Executor mirror
$(CPPTEST): tests/cpp/test_graph_executor.cpp include/fantoch_amd.hpp include/fantoch_amd.h $(LIB)
	@mkdir -p tests/cpp/build
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -o $@ tests/cpp/test_graph_executor.cpp \
	  -Lfantoch_amd -lfantoch_amd -Wl,-rpath,'$$ORIGIN/../../../fantoch_amd'

# test-only: fills the register file with tagged garbage before a kernel under
# test (tests/test_sim_poison.py)
$(POISON): tests/poison/poison.hip
	@mkdir -p tests/poison/build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -fPIC -shared -o $@ $<

# measurement helper: the handle's per-Add cost in a C++ loop (bench.py --mode handle)
$(HLAT): tools/handle_latency.cpp include/fantoch_amd.h $(LIB)
	@mkdir -p tools/build
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -o $@ tools/handle_latency.cpp \
	  -Lfantoch_amd -lfantoch_amd -Wl,-rpath,'$$ORIGIN/../../fantoch_amd'

# the host twins of the generators (table_synth_host.cpp: Tempo streams, closed-loop
# shard groups) and of the KV stage (kv_host.cpp) under AddressSanitizer and
# UBSan (slot_host.cpp, the slot executor's twins, likewise; its sessions: slot-advance-check;
# pred_host.cpp, the predecessors executor's sessions: pred-advance-check;
# pred_synth_host.cpp, the Caesar stream generator's twin: pred-synth-check;
# metrics_host.cpp, the metrics pass's twin: metrics-check; the sessions of the KV and the pending stage:
# kv-advance-check, pending-advance-check): stand-alone CPU programs, tests/cpp/NAME_check.cpp linked with the
# product source they check (not part of `all`; run them on the host only)
CHECKDIR := tests/cpp/build
$(CHECKDIR)/table_synth_host_check $(CHECKDIR)/table_group_synth_host_check: PRODUCT := fantoch_amd/csrc/table_synth_host.cpp
$(CHECKDIR)/kv_host_check $(CHECKDIR)/kv_advance_host_check: PRODUCT := fantoch_amd/csrc/kv_host.cpp
$(CHECKDIR)/pending_host_check $(CHECKDIR)/pending_advance_host_check: PRODUCT := fantoch_amd/csrc/pending_host.cpp
$(CHECKDIR)/slot_host_check $(CHECKDIR)/slot_advance_host_check: PRODUCT := fantoch_amd/csrc/slot_host.cpp
$(CHECKDIR)/pred_advance_host_check: PRODUCT := fantoch_amd/csrc/pred_host.cpp
$(CHECKDIR)/pred_synth_host_check: PRODUCT := fantoch_amd/csrc/pred_synth_host.cpp
$(CHECKDIR)/metrics_host_check: PRODUCT := fantoch_amd/csrc/metrics_host.cpp
$(CHECKDIR)/%_check: tests/cpp/%_check.cpp fantoch_amd/csrc/table_synth_host.cpp fantoch_amd/csrc/kv_host.cpp fantoch_amd/csrc/pending_host.cpp fantoch_amd/csrc/slot_host.cpp fantoch_amd/csrc/pred_host.cpp fantoch_amd/csrc/pred_synth_host.cpp fantoch_amd/csrc/metrics_host.cpp $(HDRS)
	@mkdir -p $(CHECKDIR)
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=all \
	  -Iinclude -Ifantoch_amd/csrc -o $@ $< $(PRODUCT) -lpthread
synth-check: $(CHECKDIR)/table_synth_host_check
group-synth-check: $(CHECKDIR)/table_group_synth_host_check
kv-check: $(CHECKDIR)/kv_host_check
kv-advance-check: $(CHECKDIR)/kv_advance_host_check
pending-check: $(CHECKDIR)/pending_host_check
pending-advance-check: $(CHECKDIR)/pending_advance_host_check
slot-check: $(CHECKDIR)/slot_host_check
slot-advance-check: $(CHECKDIR)/slot_advance_host_check
pred-advance-check: $(CHECKDIR)/pred_advance_host_check
pred-synth-check: $(CHECKDIR)/pred_synth_host_check
metrics-check: $(CHECKDIR)/metrics_host_check
synth-check group-synth-check kv-check kv-advance-check pending-check pending-advance-check slot-check slot-advance-check pred-advance-check pred-synth-check metrics-check:
	$<

# kernel resource usage (VGPR/SGPR/LDS/occupancy) for DESIGN.md / tuning
resource-usage:
	for f in fantoch_amd/csrc/graph_exec.hip fantoch_amd/csrc/graph_metrics.hip fantoch_amd/csrc/graph_synth.hip fantoch_amd/csrc/handle_xfer.hip fantoch_amd/csrc/graph_group.hip fantoch_amd/csrc/graph_wave.hip fantoch_amd/csrc/graph_lane.hip; do \
	  $(HIPCC) $(HIPFLAGS) -c -o /tmp/fx_ge.o $$f -Rpass-analysis=kernel-resource-usage 2>&1 \
	  | grep -E "Function Name|VGPRs:|SGPRs:|ScratchSize|Occupancy|LDS Size"; done

clean:
	rm -f $(LIB) $(ORACLE) $(CPPTEST)

.PHONY: all clean resource-usage synth-check group-synth-check kv-check kv-advance-check pending-check pending-advance-check slot-check slot-advance-check pred-advance-check pred-synth-check metrics-check
