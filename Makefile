# Build of the MI355X path-tracing integrator (no cmake needed: hipcc + g++ only).
#
#   make            libspt_hip.so (C-ABI + gfx950 kernels) and libspt_render.so (C++ render::PathTracer backend)
#   make oracle     the CPU oracle (test infrastructure, oracle/build/libcpu_ref.so), its restatement with
#                   material models (tests/cpp/libref_materials.so), the lens's device check (tests/cpp/test_device_lens)
#                   the sphere pass's (tests/cpp/test_sphere_cull), the guard-free forms' (tests/cpp/test_device_ranges)
#                   and the key minimum's (tests/cpp/test_key_min)
#   make cpp-tests  the C++ interface test driver (tests/cpp)
#
# Every float operation on the hot path is compiled with -ffp-contract=off, on the device and on the
# host, so the GPU and the CPU oracle evaluate the reference's expressions in the same order with the
# same roundings.

HIPCC  ?= /opt/rocm/bin/hipcc
CXX    ?= g++
CC     ?= gcc
ARCH   ?= gfx950

PKG    := software-path-tracer_amd
CSRC   := $(PKG)/csrc
OBJ    := $(PKG)/build
LIB    := $(PKG)/libspt_hip.so
RLIB   := $(PKG)/libspt_render.so

FPFLAGS  := -ffp-contract=off -fno-fast-math
HIPFLAGS := -O3 -fno-slp-vectorize $(FPFLAGS) -fPIC -std=c++17 --offload-arch=$(ARCH) -fno-gpu-rdc -Wall -Iinclude -I$(CSRC)
CXXFLAGS := -O2 $(FPFLAGS) -fPIC -std=c++17 -Wall -Wextra -Iinclude -I$(CSRC)

HIP_SRCS := $(CSRC)/spt_kernels.hip $(CSRC)/spt_capi.hip $(CSRC)/spt_capi_post.hip $(CSRC)/spt_jit.hip $(CSRC)/spt_denoise.hip \
            $(CSRC)/spt_reproject.hip $(CSRC)/spt_display.hip $(CSRC)/spt_noise.hip $(CSRC)/spt_denoise_guided.hip
CPP_SRCS := $(CSRC)/scene.cpp $(CSRC)/scenes.cpp $(CSRC)/spt_host.cpp
HIP_OBJS := $(patsubst $(CSRC)/%.hip,$(OBJ)/%.o,$(HIP_SRCS))
CPP_OBJS := $(patsubst $(CSRC)/%.cpp,$(OBJ)/%.o,$(CPP_SRCS))
HDRS     := include/spt.h $(wildcard $(CSRC)/*.h)

.PHONY: all oracle cpp-tests clean
all: $(LIB) $(RLIB)

$(OBJ):
	mkdir -p $(OBJ)

$(OBJ)/%.o: $(CSRC)/%.hip $(HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# run-time specialization (spt_jit.hip) compiles the kernel source it was built from: embed it
JIT_SRCS := $(CSRC)/spt_kernels.hip $(CSRC)/spt_device.h $(CSRC)/spt_kernels.h
$(OBJ)/spt_jit_src.inc: $(JIT_SRCS) scripts/embed_sources.py | $(OBJ)
	python3 scripts/embed_sources.py $@ $(JIT_SRCS)
$(OBJ)/spt_jit.o: $(CSRC)/spt_jit.hip $(OBJ)/spt_jit_src.inc $(HDRS) | $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DSPT_DEFAULT_ARCH=\"$(ARCH)\" -I$(OBJ) -c $< -o $@

$(OBJ)/%.o: $(CSRC)/%.cpp $(HDRS) | $(OBJ)
	$(CXX) $(CXXFLAGS) -c $< -o $@
# the host-only entry points: the kernels' per-pixel headers as plain C++ (HIP's headers for float4, no runtime)
$(OBJ)/spt_host.o: CXXFLAGS += -D__HIP_PLATFORM_AMD__ -I$(dir $(HIPCC))../include

$(LIB): $(HIP_OBJS) $(CPP_OBJS)
	$(HIPCC) -shared --offload-arch=$(ARCH) -fno-gpu-rdc -o $@ $^

# C++ backend implementing render::PathTracer on top of the C-ABI (host code only, plain g++)
RENDER_SRCS := $(CSRC)/HIPPathTracer.cpp $(CSRC)/RenderSettings.cpp $(CSRC)/PathTracer.cpp
$(RLIB): $(RENDER_SRCS) $(LIB) $(wildcard include/render/*.h) $(CSRC)/HIPPathTracer.h
	$(CXX) $(CXXFLAGS) -std=c++20 -shared -o $@ $(RENDER_SRCS) -L$(PKG) -lspt_hip -Wl,-rpath,'$$ORIGIN'

REFMAT := tests/cpp/libref_materials.so
DEVLENS := tests/cpp/test_device_lens
SPHCULL := tests/cpp/test_sphere_cull
DEVRANGES := tests/cpp/test_device_ranges
KEYMIN := tests/cpp/test_key_min
oracle: $(REFMAT) $(DEVLENS) $(SPHCULL) $(DEVRANGES) $(KEYMIN)

oracle/build/libcpu_ref.so: oracle/cpu_ref.c oracle/cpu_ref.h include/spt.h oracle/Makefile
	$(MAKE) -C oracle

# the integrator restated with material models (tests/test_materials_host.py, tests/test_gpu_materials.py):
# the oracle's pieces plus its own METAL / DIELECTRIC step, no product code; test infrastructure, built
# beside the C++ test drivers
$(REFMAT): tests/cpp/ref_materials.c oracle/cpu_ref.h include/spt.h oracle/build/libcpu_ref.so
	$(CC) -O2 $(FPFLAGS) -fPIC -std=c11 -Wall -Wextra -Iinclude -shared -o $@ tests/cpp/ref_materials.c \
	  -Loracle/build -lcpu_ref -lm -Wl,-rpath,'$$ORIGIN/../../oracle/build'

# GPU program (run by tests/test_gpu_lens.py; --host, run by tests/test_lens_host.py: its inputs' coverage, no
# GPU): spt_device.h's camera_lens_ray, the device build against the host build; test infrastructure, built with
# the oracle
$(DEVLENS): tests/cpp/test_device_lens.hip $(CSRC)/spt_device.h
	$(HIPCC) -O3 $(FPFLAGS) -std=c++17 --offload-arch=$(ARCH) -I$(CSRC) -o $@ $<

# GPU program (run by tests/test_gpu_sphere_cull.py; --host, run by tests/test_sphere_cull_host.py: its inputs'
# coverage, no GPU): spt_device.h's flat_sphere_pass against the loop over isect_sphere_fast; test infrastructure
$(SPHCULL): tests/cpp/test_sphere_cull.hip $(CSRC)/spt_device.h
	$(HIPCC) -O3 $(FPFLAGS) -std=c++17 --offload-arch=$(ARCH) -I$(CSRC) -o $@ $<

# GPU program (run by tests/test_gpu_flat_ranges.py): spt_device.h's guard-free forms (inv_sqrt_ranged,
# rr_divide_ranged, bounce_tangent_ranged, the path start's emission) against '/', sqrtf and the guarded forms over
# the ranges scene.cpp flat_ranges_ok admits; test infrastructure
$(DEVRANGES): tests/cpp/test_device_ranges.hip $(CSRC)/spt_device.h
	$(HIPCC) -O3 $(FPFLAGS) -std=c++17 --offload-arch=$(ARCH) -I$(CSRC) -o $@ $<

# GPU program (run by tests/test_gpu_key_min_device.py): spt_device.h's key_min against the integer minimum of two
# closest-hit keys; test infrastructure
$(KEYMIN): tests/cpp/test_key_min.hip tests/cpp/key_min_words.h $(CSRC)/spt_device.h
	$(HIPCC) -O3 $(FPFLAGS) -std=c++17 --offload-arch=$(ARCH) -I$(CSRC) -o $@ $<

cpp-tests: $(RLIB) oracle
	$(MAKE) -C tests/cpp

clean:
	rm -rf $(OBJ) $(LIB) $(RLIB)
	$(MAKE) -C oracle clean
	rm -f $(REFMAT) $(DEVLENS) $(SPHCULL) $(DEVRANGES) $(KEYMIN)
	-$(MAKE) -C tests/cpp clean
