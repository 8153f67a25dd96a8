# plain-C caller of the depth texture entry points (no HIP headers, no C++): gcc + dlopen.  make -C tests/c -f depth_texture_smoke.mk
depth_texture_smoke: depth_texture_smoke.c ../../include/swr.h
	gcc -O1 -std=c11 -Wall -Wextra -I../../include depth_texture_smoke.c -o $@ -ldl
