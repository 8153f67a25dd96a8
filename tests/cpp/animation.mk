# skeletal animation through the C++ host mirror (g++, host only; links the product library).  make -C tests/cpp -f animation.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
test_animation: test_animation.cpp $(ROOT)/softwarerenderer_amd/cpp/Rasterizer.hpp $(ROOT)/include/swr.h
	g++ -O2 -std=c++17 -I$(ROOT)/include -I$(ROOT)/softwarerenderer_amd/cpp test_animation.cpp -o $@ \
	    -L$(ROOT)/softwarerenderer_amd -lswr_hip -Wl,-rpath,$(ROOT)/softwarerenderer_amd -Wl,-rpath,/opt/rocm/lib
