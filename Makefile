# Build everything in-tree (the .so files travel to the GPU box with the
# repo snapshot; they are git-ignored).
#   make            HIP library (gfx950) + oracle (test infrastructure)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -fPIC -shared -std=c++17 -Wall

LIB = hiccl_amd/libhiccl_reduce.so

PROBE = tools/libhbm_probe.so

all: $(LIB) $(PROBE) cpp oracle

$(PROBE): tools/hbm_probe.hip
	$(HIPCC) $(HIPFLAGS) -o $@ $<

# The library: four kernel translation units over one header of templates
# (engine.h) -- reduce.hip, the SUM kernels, reduce_ops.hip, the MAX / MIN
# kernels, reduce_prod.hip, the PROD and bitwise kernels, and reduce_scale.hip,
# the scaled sums, which also takes in reduce_f8.hip, the OCP FP8 types, and
# reduce_widen.hip, the widened sums, reduce_accum.hip, the accumulating
# ones, reduce_mixed.hip, the mixed plan kernels, and reduce_weighted.hip, the
# weighted widened sums (the library keeps four code objects, the
# scaled sums' last), compiled side by
# side (reduce.hip the longest) -- and the host files (seconds each), as
# objects under build/obj, linked once.  The link order is the order of the
# library's code objects: the SUM unit first, new units last.
# Both are compiled by hipcc's clang at -O3 without fast-math (the AUTO rules
# compare doubles) and without per-thread default streams; the host files as
# plain C++, so they carry no device code.
CSRC = hiccl_amd/csrc
OBJDIR = build/obj
OBJFLAGS = -O3 -fPIC -std=c++17 -Wall -MMD -MP
LIB_HOST = runtime policy oneshot plan host_pipe signal program util
LIB_KERNELS = reduce reduce_ops reduce_prod reduce_scale
LIB_OBJS = $(LIB_KERNELS:%=$(OBJDIR)/%.o) $(LIB_HOST:%=$(OBJDIR)/%.o)

# The atomic optimizer rewrites the one-lane unit-ticket grab into a
# wave-reduction whose result is read back at once (s_waitcnt vmcnt(0) at the
# top of every unit); without it the wait lands after the unit's last add.
LIBFLAGS = -mllvm -amdgpu-atomic-optimizer-strategy=None

$(OBJDIR)/%.o: $(CSRC)/%.hip
	@mkdir -p $(OBJDIR)
	$(HIPCC) --offload-arch=$(ARCH) $(OBJFLAGS) $(LIBFLAGS) -c -o $@ $<

$(OBJDIR)/%.o: $(CSRC)/%.cpp
	@mkdir -p $(OBJDIR)
	$(HIPCC) -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include $(OBJFLAGS) -c -o $@ $<

$(LIB): $(LIB_OBJS) $(CSRC)/exports.map
	$(HIPCC) --offload-arch=$(ARCH) -fPIC -shared -Wl,--version-script=$(CSRC)/exports.map -o $@ $(LIB_OBJS)

-include $(LIB_OBJS:.o=.d)

# oracle/_ref/collectives_main_hip links the HIP library: build it first
oracle: $(LIB)
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(LIB_OBJS) $(LIB_OBJS:.o=.d)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean

# ---- C++ surface (include/hiccl.h): drivers and test tools -----------------
MPI_INC ?= /opt/conda/include
MPI_LIB ?= /opt/conda/lib
CXX ?= g++
CXXFLAGS = -std=c++17 -O2 -Wall -Wno-unused-function -Iinclude -I$(MPI_INC)
MPI_LINK = $(MPI_LIB)/libmpi.so -Wl,-rpath,/usr/lib/x86_64-linux-gnu:$(MPI_LIB)
# the XCCL level runs on RCCL point-to-point (include/hiccl/transport.h)
HIP_HOST = -D__HIP_PLATFORM_AMD__ -DHICCL_WITH_RCCL -I/opt/rocm/include
HIP_LINK = -Lhiccl_amd -lhiccl_reduce -Wl,-rpath,'$$ORIGIN/../hiccl_amd' -L/opt/rocm/lib -lamdhip64 -lrccl -Wl,-rpath,/opt/rocm/lib
ABI_LINK = -Lhiccl_amd -lhiccl_reduce -Wl,-rpath,'$$ORIGIN/../hiccl_amd' -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
HDRS = include/hiccl.h $(wildcard include/hiccl/*.h) include/hiccl_reduce.h hiccl_amd/csrc/compose.h

CPP_BINS = build/plan_dump build/collectives_host build/collectives_host_f32 build/collectives_hip build/collectives_hip_f32 \
           build/readme_example_host build/readme_example_hip build/abi_c build/ipc_reuse build/sync_wait_probe \
           build/f16_add build/f16_compute_host build/f16_compute_hip \
           build/ops_add build/ops_compute_host build/ops_compute_hip build/ops_comm_host build/ops_comm_hip \
           build/prod_add build/prod_compute_host build/prod_compute_hip build/prod_comm_host build/prod_comm_hip \
           build/scale_finish build/scale_compute_host build/scale_compute_hip \
           build/f8_add build/f8_compute_host build/f8_compute_hip \
           build/types_comm_host build/types_comm_hip \
           build/widen_sum build/widen_sum_hip \
           build/accum_sum build/accum_sum_hip \
           build/avg_comm_host build/avg_comm_hip \
           build/weighted_sum build/weighted_sum_hip

cpp: $(CPP_BINS)

build/plan_dump: tests/cpp/plan_dump.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $< $(MPI_LINK)

build/collectives_host: hiccl_amd/csrc/collectives.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/collectives_host_f32: hiccl_amd/csrc/collectives.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -DHICCL_DRIVER_FLOAT -o $@ $< $(MPI_LINK)

build/collectives_hip: hiccl_amd/csrc/collectives.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

build/collectives_hip_f32: hiccl_amd/csrc/collectives.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -DHICCL_DRIVER_FLOAT -o $@ $< $(HIP_LINK) $(MPI_LINK)

build/readme_example_host: hiccl_amd/csrc/readme_example.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/readme_example_hip: hiccl_amd/csrc/readme_example.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# two-process reproducer of the IPC close/reopen behaviour (tests/test_ipc_reuse_gpu.py)
build/ipc_reuse: tests/cpp/ipc_reuse.cpp include/hiccl_reduce.h $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(ABI_LINK) $(MPI_LINK)

# host wait after a C5-step launch, from C++ (tools/sync_wait_probe.cpp)
build/sync_wait_probe: tools/sync_wait_probe.cpp include/hiccl_reduce.h $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -o $@ $< $(ABI_LINK)

# HiCCL::f16: `+=` on every bit pattern (host), and Compute<f16> on the host
# port and on the GPU (tests/test_f16_cpu.py, tests/test_f16_gpu.py)
build/f16_add: tests/cpp/f16_add.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/f16_compute_host: tests/cpp/f16_compute.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/f16_compute_hip: tests/cpp/f16_compute.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# HiCCL::maxof / minof (include/hiccl/ops.h): `+=` against the NumPy
# restatement (host), and Compute<maxof<float>> / Compute<minof<bf16>> on the
# host port and on the GPU (tests/test_ops_cpu.py, tests/test_ops_gpu.py)
build/ops_add: tests/cpp/ops_add.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/ops_compute_host: tests/cpp/ops_compute.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/ops_compute_hip: tests/cpp/ops_compute.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Comm<maxof<float>>: a reduce to root under MPI (tests/test_ops_cpu.py host, tests/test_ops_gpu.py GPU)
build/ops_comm_host: tests/cpp/ops_comm.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/ops_comm_hip: tests/cpp/ops_comm.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# HiCCL::prodof / bandof / borof / bxorof (include/hiccl/ops.h): `+=` against
# the exact product rounded once (a stand-alone host program), Compute<prodof<
# float>> / Compute<prodof<bf16>> and Comm<prodof<float>> / Comm<bxorof<
# uint64_t>> on the host port and on the GPU (tests/test_prod_cpu.py,
# tests/test_prod_gpu.py)
build/prod_add: tests/cpp/prod_add.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $<

build/prod_compute_host: tests/cpp/prod_compute.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/prod_compute_hip: tests/cpp/prod_compute.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

build/prod_comm_host: tests/cpp/prod_comm.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/prod_comm_hip: tests/cpp/prod_comm.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Scaled sums: HiCCL::scale_finish<T> against the exact product rounded twice
# (a stand-alone host program), Compute<float> / Compute<bf16> with set_scale
# on the host port and on the GPU (tests/test_scale_cpu.py,
# tests/test_scale_gpu.py)
build/scale_finish: tests/cpp/scale_finish.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $<

build/scale_compute_host: tests/cpp/scale_compute.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/scale_compute_hip: tests/cpp/scale_compute.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# OCP FP8: HiCCL::f8e4m3 / f8e5m2 -- `+=`, round, operator float and the
# maxof / minof identities as tables (a stand-alone host program), and
# Compute<f8e4m3> / Compute<f8e5m2>, plain and with set_scale, on the host port
# and on the GPU (tests/test_f8_cpu.py, tests/test_f8_gpu.py)
build/f8_add: tests/cpp/f8_add.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $<

build/f8_compute_host: tests/cpp/f8_compute.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/f8_compute_hip: tests/cpp/f8_compute.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Comm<T> for every element type and operator wrapper: the eight collectives
# on raw bytes, judged by tests/comm_expected.py (tests/test_types_comm_cpu.py,
# tests/test_types_comm_gpu.py)
build/types_comm_host: tests/cpp/types_comm.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/types_comm_hip: tests/cpp/types_comm.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Widened sums: HiCCL::WidenCompute<T> (bf16, f16, f8e4m3, f8e5m2 inputs, float
# outputs) on the host port -- a stand-alone program that tests/test_widen_cpu.py
# also builds with sanitizers -- and on the GPU (tests/test_widen_gpu.py)
build/widen_sum: tests/cpp/widen_sum.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/widen_sum_hip: tests/cpp/widen_sum.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Accumulating widened sums: WidenCompute<T>::set_accumulate (out += alpha *
# sum) on the host port -- a stand-alone program that tests/test_accum_cpu.py
# also builds with sanitizers -- and on the GPU (tests/test_accum_gpu.py)
build/accum_sum: tests/cpp/accum_sum.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/accum_sum_hip: tests/cpp/accum_sum.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Averaging Comm<T>: types_comm's driver with Comm<T>::set_scale(alpha) before
# the collective is composed (tests/test_avg_comm_cpu.py, tests/test_avg_comm_gpu.py)
build/avg_comm_host: tests/cpp/avg_comm.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/avg_comm_hip: tests/cpp/avg_comm.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# Weighted widened sums: WidenCompute<T>::add with per-input weights on the
# host port -- a stand-alone program that tests/test_weighted_cpu.py also builds
# with sanitizers -- and on the GPU (tests/test_weighted_gpu.py)
build/weighted_sum: tests/cpp/weighted_sum.cpp $(HDRS)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -fopenmp -DHICCL_PORT_HOST -o $@ $< $(MPI_LINK)

build/weighted_sum_hip: tests/cpp/weighted_sum.cpp $(HDRS) $(LIB)
	@mkdir -p build
	$(CXX) $(CXXFLAGS) $(HIP_HOST) -o $@ $< $(HIP_LINK) $(MPI_LINK)

# plain C99 client of the C ABI (the header must stay C)
build/abi_c: tests/cpp/abi_c.c include/hiccl_reduce.h $(LIB)
	@mkdir -p build
	gcc -std=c99 -pedantic -Wall -Wextra -Werror -Iinclude -o $@ $< $(ABI_LINK)

.PHONY: cpp
