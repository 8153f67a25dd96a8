# the deforming-mesh calls through the C++ host mirror (g++, host only; links the product library).  make -C tests/cpp -f mesh_deform.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
test_mesh_deform: test_mesh_deform.cpp $(ROOT)/softwarerenderer_amd/cpp/Rasterizer.hpp $(ROOT)/include/swr.h
	g++ -O2 -std=c++17 -I$(ROOT)/include -I$(ROOT)/softwarerenderer_amd/cpp test_mesh_deform.cpp -o $@ \
	    -L$(ROOT)/softwarerenderer_amd -lswr_hip -Wl,-rpath,$(ROOT)/softwarerenderer_amd -Wl,-rpath,/opt/rocm/lib
